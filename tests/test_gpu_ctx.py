"""The context API (layer (B) of include/abub_hip.h: the abub_ctx_* calls, the drop-in boundary of DESIGN.md section 1)
called directly, every entry point against the CPU oracle or plain numpy, bit for bit.

The host library reaches the contexts in one narrow way (first = 1, (i, ref) = (0, 1), cap = 65536, one context per
thread).  Here every argument takes the values the header allows: any first / count / ref_offset, both orders of
(i, ref), ROIs on every border, any cap, training sets on both sides of max_frames, refused calls that must leave the
context as it was, several contexts at work at once.  Every reference image that is not meant to be zero is asserted
to have non-zero pixels, so that an all-zero result cannot pass by accident.  Every refusal here is one the library
makes before it launches anything."""
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from autobub3hs_amd import _lib  # noqa: E402

from ctxapi import E_INVALID, E_OVERFLOW, OK, SENT, Ctx  # noqa: E402
from test_bellows_batched import exact_terms  # noqa: E402
from test_gpu_knobs import _defaults  # noqa: E402,F401  (autouse: default K2 / K3 options after every test)

# (W, H, fast path): which K2 / K3 kernels a context of this shape runs
SHAPES = [
    (1280, 64, 1),  # NDW 5 fast path
    (1680, 50, 1),  # NDW 7, 60 lanes
    (100, 33, 1),   # NDW 1, 25 lanes
    (322, 37, 0),   # generic, W % 4 != 0
    (268, 20, 0),   # generic although W % 4 == 0 (W / 4 = 67 lanes of one dword)
    (2052, 9, 0),   # generic, W > 2048
    (5, 3, 0),      # degenerate
]
SHAPE_IDS = ["%dx%d" % (w, h) for w, h, _ in SHAPES]
shapes = pytest.mark.parametrize("W,H", [(w, h) for w, h, _ in SHAPES], ids=SHAPE_IDS)


def test_shapes_take_the_stated_paths():
    L = _lib.lib()
    for W, H, fast in SHAPES:
        assert L.abub_fast_path(W) == fast, W
    assert L.abub_fast_path(1680) == 1 and L.abub_fast_path(536) == 0  # the full-size case; 2 * 268


# ------------------------------------------------------------------------------------------------------------------
# inputs and references
# ------------------------------------------------------------------------------------------------------------------
def make_stack(W, H, F, seed, amp=12):
    """Base plus noise, and from the middle frame on a bright disc (a bubble) a third of the way across."""
    rs = np.random.RandomState(seed)
    base = rs.randint(30, 200, (H, W))
    fr = base[None] + rs.randint(-amp, amp + 1, (F, H, W))
    yy, xx = np.mgrid[:H, :W]
    r = max(min(W, H) // 4, 1)
    disc = (yy - H // 2) ** 2 + (xx - W // 3) ** 2 <= r * r
    fr[F // 2:, disc] += 70
    return np.clip(fr, 0, 255).astype(np.uint8), base


def make_model(W, H, base, seed, saturated=False):
    """sigma in 0..2; the saturated model has sigma >= 43 (6 * sigma > 255) on about half of the pixels."""
    rs = np.random.RandomState(seed + 1)
    mu = np.clip(base + rs.randint(-3, 4, (H, W)), 0, 255).astype(np.uint8)
    sigma = rs.randint(0, 3, (H, W)).astype(np.uint8)
    if saturated:
        big = rs.rand(H, W) < 0.5
        sigma[big] = rs.randint(43, 256, (H, W))[big]
    return mu, sigma


def make_image(W, H, seed):
    """An image with every kind of value: zeros, 254, 255 and noise."""
    rs = np.random.RandomState(seed + 2)
    img = rs.randint(0, 256, (H, W))
    img[rs.rand(H, W) < 0.3] = 0
    img.ravel()[0] = 255
    img.ravel()[-1] = 254
    img.ravel()[(W * H) // 2] = 0
    return img.astype(np.uint8)


def sat_sub(a, b):
    return np.clip(a.astype(int) - b.astype(int), 0, 255).astype(np.uint8)


def nonzero(img, what=""):
    """The oracle's image has something in it (an all-zero result must not be able to pass)."""
    assert np.count_nonzero(img) > 0, what
    return img


def check_foreground(ctx, img, thr):
    """abub_ctx_foreground with cap = the true count lists exactly the pixels of img above thr."""
    exp = np.flatnonzero(img.ravel() > thr)
    rc, n, idx = ctx.foreground(thr, max(len(exp), 1))
    assert rc == OK and n == len(exp), (rc, n, len(exp), thr)
    assert np.array_equal(np.sort(idx[:n]), exp), thr
    assert np.all(idx[n:] == SENT)


def check_current(ctx, img, thr=0):
    """The context's current image is `img`: through abub_ctx_fetch_image and through abub_ctx_foreground."""
    rc, got = ctx.fetch_image()
    assert rc == OK and np.array_equal(got, img)
    check_foreground(ctx, img, thr)


def loaded(W, H, F, seed, saturated=False, max_frames=None):
    """A context with a model set and a stack of F frames uploaded -> ctx, frames, mu, sigma."""
    fr, base = make_stack(W, H, F, seed)
    mu, sigma = make_model(W, H, base, seed, saturated)
    ctx = Ctx(W, H, max_frames or F)
    assert ctx.set_model(mu, sigma) == OK
    assert ctx.upload(list(fr)) == OK
    return ctx, fr, mu, sigma


# ------------------------------------------------------------------------------------------------------------------
# abub_ctx_diff_hist_batch
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("saturated", [False, True], ids=["sigma0-2", "sigma6-saturates"])
@shapes
def test_diff_hist_batch_any_first_count_offset(oracle, W, H, saturated):
    F = 7  # ref_offset F + 1 = 8 is the largest stride the chained scan takes
    ctx, fr, mu, sigma = loaded(W, H, F, 11 * W + H, saturated)
    with ctx:
        for off in (0, 1, 2, 3, F + 1):
            ref = np.stack([oracle.hist256(oracle.process_frame(fr[i], fr[max(i - off, 0)], sigma)) for i in range(F)])
            if off == 0:
                assert np.all(ref[:, 0] == W * H)  # a frame against itself
            else:
                left = ref[1:, 0] < W * H  # every other pair leaves something (of 15 pixels, most pairs do)
                assert np.all(left) if W * H >= 100 else left.sum() > len(left) // 2, off
            for first in (0, 1, 5):
                for count in range(1, F - first + 1):
                    rc, h = ctx.batch(off, first, count, rows=count + 1)
                    assert rc == OK, (off, first, count)
                    assert np.array_equal(h[:count], ref[first:first + count]), (off, first, count)
                    assert np.all(h[count] == SENT), (off, first, count)  # nothing past [count][256]


def test_diff_hist_batch_count_zero_and_refusals(oracle):
    W, H, F = 100, 33, 6
    fr, base = make_stack(W, H, F, 5)
    mu, sigma = make_model(W, H, base, 5)
    L = _lib.lib()
    with Ctx(W, H, F) as ctx:
        assert ctx.batch(1, 0, 1)[0] == E_INVALID  # neither model nor stack
        assert ctx.upload(list(fr)) == OK
        assert ctx.batch(1, 0, 1)[0] == E_INVALID and b"no model" in L.abub_last_error()
    with Ctx(W, H, F) as ctx:
        assert ctx.set_model(mu, sigma) == OK
        assert ctx.batch(1, 0, 1)[0] == E_INVALID  # no stack
        assert ctx.upload(list(fr)) == OK
        for first in (0, 3, F):
            rc, h = ctx.batch(2, first, 0, rows=2)
            assert rc == OK and np.all(h == SENT), first  # count = 0: fine, hist_out untouched
        for off, first, count in ((1, 0, F + 1), (1, 1, F), (1, F, 1), (1, F + 1, 0), (-1, 0, 1), (1, -1, 1), (1, 0, -1),
                                  (1, -1, F + 1)):
            rc, h = ctx.batch(off, first, count, rows=F + 2)
            assert rc == E_INVALID and np.all(h == SENT), (off, first, count)
        assert b"abub_ctx_diff_hist_batch" in L.abub_last_error()
        # the refusals changed nothing
        rc, h = ctx.batch(2, 1, F - 1)
        assert rc == OK
        for k, i in enumerate(range(1, F)):
            assert np.array_equal(h[k], oracle.hist256(nonzero(oracle.process_frame(fr[i], fr[max(i - 2, 0)], sigma))))


# ------------------------------------------------------------------------------------------------------------------
# abub_ctx_diff_frame
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("saturated", [False, True], ids=["sigma0-2", "sigma6-saturates"])
@shapes
def test_diff_frame_orders_and_null_outputs(oracle, W, H, saturated):
    F = 5
    ctx, fr, mu, sigma = loaded(W, H, F, 13 * W + H, saturated)
    with ctx:
        for i, ref in ((4, 1), (2, 2), (1, 4), (3, 2), (0, 4)):
            D = oracle.process_frame(fr[i], fr[ref], sigma)
            if i != ref:
                nonzero(D, (i, ref))
            else:
                assert not D.any()
            href = oracle.hist256(D)
            for want_D, want_hist in ((True, True), (False, True), (True, False), (False, False)):
                assert ctx.set_image(make_image(W, H, i)) == OK  # the call must replace this
                rc, Dg, hg = ctx.diff_frame(i, ref, want_D, want_hist)
                assert rc == OK, (i, ref)
                if want_D:
                    assert np.array_equal(Dg, D), (i, ref)
                if want_hist:
                    assert np.array_equal(hg, href), (i, ref)
                check_current(ctx, D)
        for i, ref in ((F, 0), (0, F), (-1, 0), (0, -1)):
            assert ctx.diff_frame(i, ref)[0] == E_INVALID, (i, ref)
        check_current(ctx, D)  # a refused call leaves the current image


# ------------------------------------------------------------------------------------------------------------------
# abub_ctx_diff_frame_roi
# ------------------------------------------------------------------------------------------------------------------
def rois_of(W, H, hot):
    """ROIs on every border and corner, 1x1 and a one-column strip through the pixel `hot` (x, y), the whole frame."""
    w, h = max(min(W - 1, 37), 1), max(min(H - 1, 11), 1)
    mx, my = (W - w) // 2, (H - h) // 2
    hx, hy = hot
    return [
        (0, 0, w, h), (W - w, 0, w, h), (0, H - h, w, h), (W - w, H - h, w, h),   # corners
        (mx, 0, w, h), (mx, H - h, w, h), (0, my, w, h), (W - w, my, w, h),       # one border each
        (0, hy, W, 1), (0, 0, W, min(H, 2)), (0, H - 1, W, 1), (W - 1, 0, 1, H),  # full-width rows, the last column
        (hx, hy, 1, 1), (hx, 0, 1, H), (0, 0, W, H),
    ]


@shapes
def test_diff_frame_roi_both_orders_borders_and_refusals(oracle, W, H):
    F = 5
    ctx, fr, mu, sigma = loaded(W, H, F, 17 * W + H, saturated=False)
    with ctx:
        i, ref = 1, 4
        # a pixel where the thresholded difference itself is non-zero: a 1x1 ROI there cannot be zero
        m = np.abs(fr[i].astype(int) - fr[ref].astype(int)) - 6 * sigma.astype(int)
        hy, hx = np.unravel_index(np.argmax(m), m.shape)
        assert m[hy, hx] > 0
        for roi in rois_of(W, H, (int(hx), int(hy))):
            for a, b in ((i, ref), (ref, i)):  # ref > i, and ref < i: the swapped call
                D = nonzero(oracle.process_frame(fr[a], fr[b], sigma, roi=roi), roi)
                rx, ry, rw, rh = roi
                outside = D.copy()
                outside[ry:ry + rh, rx:rx + rw] = 0
                assert not outside.any()
                rc, Dg, hg = ctx.diff_frame_roi(a, b, roi)
                assert rc == OK, (roi, a, b)
                assert np.array_equal(Dg, D), (roi, a, b)
                assert np.array_equal(hg, oracle.hist256(D)), (roi, a, b)
            check_current(ctx, D)
        # null outputs in turn
        roi = (0, 0, W, H)
        D = oracle.process_frame(fr[ref], fr[i], sigma, roi=roi)
        rc, Dg, hg = ctx.diff_frame_roi(ref, i, roi, want_D=False)
        assert rc == OK and Dg is None and np.array_equal(hg, oracle.hist256(D))
        rc, Dg, hg = ctx.diff_frame_roi(ref, i, roi, want_hist=False)
        assert rc == OK and hg is None and np.array_equal(Dg, D)
        # an empty ROI is an all-zero image
        for roi in ((W // 2, H // 2, 0, 1), (0, 0, 0, 0), (W - 1, H - 1, 1, 0)):
            assert ctx.set_image(make_image(W, H, 3)) == OK
            rc, Dg, hg = ctx.diff_frame_roi(ref, i, roi)
            assert rc == OK and not Dg.any() and hg[0] == W * H and not hg[1:].any(), roi
            check_current(ctx, np.zeros((H, W), np.uint8), thr=-1)
        # ROIs that leave the frame are refused and leave the current image
        img = make_image(W, H, 4)
        assert ctx.set_image(img) == OK
        for roi in ((W - 1, 0, 2, 1), (0, H - 1, 1, 2), (-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, W + 1, 1), (0, 0, 1, H + 1),
                    (W, 0, 1, 1), (0, 0, -1, 1)):
            for a, b in ((i, ref), (ref, i)):
                assert ctx.diff_frame_roi(a, b, roi)[0] == E_INVALID, roi
        assert ctx.diff_frame_roi(F, 0, (0, 0, 1, 1))[0] == E_INVALID
        check_current(ctx, img)


# ------------------------------------------------------------------------------------------------------------------
# abub_ctx_posttrig
# ------------------------------------------------------------------------------------------------------------------
@shapes
def test_posttrig_every_frame_and_saturated_model(oracle, W, H):
    F = 4
    ctx, fr, mu, sigma = loaded(W, H, F, 19 * W + H)
    rs = np.random.RandomState(W + H)
    # saturated model: mu 0 / 255, sigma on both sides of the point where 6 * sigma saturates (42 -> 252, 43 -> 255)
    mu_s = (255 * ((np.add.outer(np.arange(H), np.arange(W)) // 3) % 2)).astype(np.uint8)
    sg_s = rs.choice(np.array([0, 42, 43, 255], np.uint8), (H, W))
    with ctx:
        for m, s in ((mu, sigma), (mu_s, sg_s)):
            assert ctx.set_model(m, s) == OK
            for i in range(F):
                O = nonzero(oracle.posttrig_frame(fr[i], m, s), i)
                assert ctx.set_image(make_image(W, H, i)) == OK
                rc, Og, hg = ctx.posttrig(i)
                assert rc == OK and np.array_equal(Og, O), i
                assert np.array_equal(hg, oracle.hist256(O)), i
                check_current(ctx, O, thr=int(np.median(O)))
            rc, Og, hg = ctx.posttrig(1, want_O=False)
            O = oracle.posttrig_frame(fr[1], m, s)
            assert rc == OK and np.array_equal(hg, oracle.hist256(O))
            rc, Og, hg = ctx.posttrig(2, want_hist=False)
            assert rc == OK and np.array_equal(Og, oracle.posttrig_frame(fr[2], m, s))
        assert ctx.posttrig(F)[0] == E_INVALID and ctx.posttrig(-1)[0] == E_INVALID


# ------------------------------------------------------------------------------------------------------------------
# current image: set / fetch / subtract / foreground
# ------------------------------------------------------------------------------------------------------------------
@shapes
def test_set_fetch_subtract_image(oracle, W, H):
    with Ctx(W, H, 1) as ctx:  # no model, no stack: these calls need neither
        img = nonzero(make_image(W, H, 7))
        assert ctx.set_image(img) == OK
        check_current(ctx, img)
        sub = np.random.RandomState(W).randint(0, 200, (H, W)).astype(np.uint8)
        exp = nonzero(sat_sub(img, sub))
        assert (exp == 0).sum() > (img == 0).sum()  # the subtraction saturates somewhere
        rc, h = ctx.subtract_image(sub)
        assert rc == OK and np.array_equal(h, oracle.hist256(exp))
        check_current(ctx, exp)
        exp2 = sat_sub(exp, np.full((H, W), 255, np.uint8))  # everything saturates to zero
        rc, h = ctx.subtract_image(np.full((H, W), 255, np.uint8))
        assert rc == OK and h[0] == W * H and not h[1:].any() and not exp2.any()
        check_current(ctx, exp2, thr=-1)


@shapes
def test_foreground_thresholds_and_caps(W, H):
    P = W * H
    with Ctx(W, H, 1) as ctx:
        img = make_image(W, H, 9)
        assert ctx.set_image(img) == OK
        for thr in (-1, 0, 100, 254, 255):
            exp = np.flatnonzero(img.ravel() > thr)
            if thr == -1:
                assert len(exp) == P  # every pixel, the zeros too
            assert (len(exp) == 0) == (thr == 255)
            check_foreground(ctx, img, thr)                      # cap = the count
            rc, n, idx = ctx.foreground(thr, P + 3)              # cap above anything the image can hold
            assert rc == OK and n == len(exp) and np.array_equal(np.sort(idx[:n]), exp) and np.all(idx[n:] == SENT)
            if len(exp) > 1:                                     # cap one below: the true count, cap valid indices
                cap = len(exp) - 1
                rc, n, idx = ctx.foreground(thr, cap)
                assert rc == E_OVERFLOW and n == len(exp), (thr, rc, n)
                assert len(np.unique(idx)) == cap and np.all(np.isin(idx, exp)), thr
        exp = np.flatnonzero(img.ravel() > 0)
        rc, n, idx = ctx.foreground(0, 1)
        assert rc == E_OVERFLOW and n == len(exp) and idx[0] in exp
        assert ctx.foreground(0, 0)[0] == E_INVALID and ctx.foreground(0, -5)[0] == E_INVALID


def test_foreground_caps_above_65536():
    """70000 foreground pixels in a 1280 x 64 frame: the header promises ABUB_E_OVERFLOW iff *n > cap, for any cap."""
    W, H, NFG = 1280, 64, 70000
    rs = np.random.RandomState(70000)
    img = np.zeros(W * H, np.uint8)
    where = rs.permutation(W * H)[:NFG]
    img[where] = rs.randint(11, 256, NFG)
    img[rs.permutation(W * H)[NFG:NFG + 5000]] = 10  # at the threshold: not foreground
    img[where] = np.maximum(img[where], 11)
    thr = 10
    exp = np.flatnonzero(img > thr)
    assert len(exp) == NFG
    img = img.reshape(H, W)
    with Ctx(W, H, 1) as ctx:
        assert ctx.set_image(img) == OK
        for cap in (65536, 100000, NFG, 65536, W * H, 2 * W * H):  # (and back to the small buffer after it grew)
            rc, n, idx = ctx.foreground(thr, cap)
            if cap >= NFG:
                assert rc == OK and n == NFG, (cap, rc, n)
                assert np.array_equal(np.sort(idx[:NFG]), exp), cap
                assert np.all(idx[NFG:] == SENT), cap
            else:
                assert rc == E_OVERFLOW and n == NFG, (cap, rc, n)
                assert len(np.unique(idx)) == cap and np.all(np.isin(idx, exp)), cap
        rc, n, idx = ctx.foreground(thr, NFG - 1)
        assert rc == E_OVERFLOW and n == NFG, (rc, n)
        assert len(np.unique(idx)) == NFG - 1 and np.all(np.isin(idx, exp))
        check_current(ctx, img, thr=-1)  # all 81920 pixels


# ------------------------------------------------------------------------------------------------------------------
# abub_ctx_train / abub_ctx_pair_hist / abub_ctx_upload_stack
# ------------------------------------------------------------------------------------------------------------------
@shapes
def test_train_on_both_sides_of_max_frames(oracle, W, H):
    MAXF, F = 4, 4
    fr, base = make_stack(W, H, F, 23 * W + H)
    other_mu = np.zeros((H, W), np.uint8)
    other_sigma = np.full((H, W), 255, np.uint8)  # under this model every D is zero
    with Ctx(W, H, MAXF) as ctx:
        for N in (1, 2, MAXF, MAXF + 1, 3 * MAXF):
            rs = np.random.RandomState(N + W)
            tr = np.clip(base[None] + rs.randint(-2, 3, (N, H, W)), 0, 255).astype(np.uint8)
            mu_r, sg_r = oracle.welford(tr)
            assert ctx.set_model(other_mu, other_sigma) == OK
            assert ctx.upload(list(fr)) == OK
            assert ctx.diff_frame(3, 0)[0] == OK
            rc, mu, sg = ctx.train(list(tr))
            assert rc == OK, N
            assert np.array_equal(mu, mu_r) and np.array_equal(sg, sg_r), N
            # the resident stack is gone, on both paths
            assert ctx.diff_frame(3, 0)[0] == E_INVALID, N
            assert ctx.posttrig(0)[0] == E_INVALID and ctx.batch(1, 0, 1)[0] == E_INVALID, N
            # and the trained model is the context's model
            assert ctx.upload(list(fr)) == OK
            D = nonzero(oracle.process_frame(fr[3], fr[0], sg_r), N)
            rc, Dg, hg = ctx.diff_frame(3, 0)
            assert rc == OK and np.array_equal(Dg, D) and np.array_equal(hg, oracle.hist256(D)), N
            O = nonzero(oracle.posttrig_frame(fr[2], mu_r, sg_r), N)
            rc, Og, hg = ctx.posttrig(2)
            assert rc == OK and np.array_equal(Og, O) and np.array_equal(hg, oracle.hist256(O)), N
        # a null pointer among the frames is refused before anything is copied: model and stack stay
        for N, k in ((3, 1), (MAXF + 2, MAXF)):
            bad = [tr[j % len(tr)] for j in range(N)]
            bad[k] = None
            rc, mu, sg = ctx.train(bad)
            assert rc == E_INVALID and np.all(mu == 0xA5) and np.all(sg == 0xA5), (N, k)
            rc, Dg, hg = ctx.diff_frame(3, 0)
            assert rc == OK and np.array_equal(Dg, D), (N, k)
        assert ctx.train([])[0] == E_INVALID


@shapes
def test_pair_hist_and_what_it_invalidates(oracle, W, H):
    ctx, fr, mu, sigma = loaded(W, H, 3, 29 * W + H)
    with ctx:
        assert ctx.diff_frame(2, 0)[0] == OK
        for a, b in ((0, 2), (2, 0), (1, 1)):
            d = sat_sub(fr[b], fr[a])
            if a != b:
                nonzero(d)
            rc, h = ctx.pair_hist(fr[a], fr[b])
            assert rc == OK and np.array_equal(h, oracle.hist256(d)), (a, b)
        zeros = np.zeros((H, W), np.uint8)  # the host's use: the histogram of an image
        rc, h = ctx.pair_hist(zeros, fr[1])
        assert rc == OK and np.array_equal(h, oracle.hist256(fr[1]))
        assert ctx.diff_frame(2, 0)[0] == E_INVALID  # the slab was used: no resident stack
        assert ctx.upload(list(fr)) == OK
        D = nonzero(oracle.process_frame(fr[2], fr[0], sigma))  # the model stayed
        rc, Dg, hg = ctx.diff_frame(2, 0)
        assert rc == OK and np.array_equal(Dg, D)
    with Ctx(W, H, 1) as one:
        assert one.pair_hist(fr[0], fr[1])[0] == E_INVALID  # needs room for two frames


def test_upload_stack_refusals_leave_the_stack(oracle):
    W, H, F = 268, 20, 5
    ctx, fr, mu, sigma = loaded(W, H, F, 31, max_frames=F)
    new, _ = make_stack(W, H, F, 32)
    assert not np.array_equal(new[0], fr[0])
    L = _lib.lib()
    with ctx:
        def old_stack_serves():
            for i, ref in ((4, 0), (1, 0), (0, 3), (2, 1)):
                D = nonzero(oracle.process_frame(fr[i], fr[ref], sigma))
                rc, Dg, hg = ctx.diff_frame(i, ref)
                assert rc == OK and np.array_equal(Dg, D) and np.array_equal(hg, oracle.hist256(D)), (i, ref)
            rc, h = ctx.batch(1, 0, F)
            assert rc == OK
            for i in range(F):
                assert np.array_equal(h[i], oracle.hist256(oracle.process_frame(fr[i], fr[max(i - 1, 0)], sigma))), i

        old_stack_serves()
        assert ctx.upload(list(new) + [new[0]]) == E_INVALID  # F > max_frames
        assert b"max_frames" in L.abub_last_error()
        assert ctx.upload(list(new), F=0) == E_INVALID and ctx.upload(list(new), F=-1) == E_INVALID
        old_stack_serves()
        for k in (2, F - 1, 0):  # a null pointer in the middle, at the end, in front
            bad = list(new)
            bad[k] = None
            assert ctx.upload(bad) == E_INVALID, k
            assert b"null frame" in L.abub_last_error()
            old_stack_serves()
        # a shorter stack replaces the old one: F follows
        assert ctx.upload(list(new[:2])) == OK
        assert ctx.diff_frame(2, 0)[0] == E_INVALID
        D = nonzero(oracle.process_frame(new[1], new[0], sigma))
        rc, Dg, hg = ctx.diff_frame(1, 0)
        assert rc == OK and np.array_equal(Dg, D)


# ------------------------------------------------------------------------------------------------------------------
# abub_ctx_match_template
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(100, 33), (268, 20), (5, 3)], ids=["100x33", "268x20", "5x3"])
def test_match_template_sizes_and_saturation(W, H):
    rs = np.random.RandomState(W * H)
    fr = rs.randint(0, 256, (3, H, W)).astype(np.uint8)
    fr[2] = 255
    with Ctx(W, H, 3) as ctx:  # needs no model
        assert ctx.upload(list(fr)) == OK
        sizes = {(1, 1), (W, H), (min(7, W), min(5, H)), (min(31, W), 3), (1, H), (W, 1), (W - 1, H - 1)}
        for tw, th in sorted(s for s in sizes if s[0] > 0 and s[1] > 0):
            tmpl = rs.randint(1, 256, (th, tw)).astype(np.uint8)
            for i in (0, 1):
                en, ew = exact_terms(fr[i], tmpl)
                assert en.any() and ew.any()
                rc, num, w2 = ctx.match_template(i, tmpl)
                assert rc == OK, (tw, th, i)
                assert np.array_equal(num, en) and np.array_equal(w2, ew), (tw, th, i)
            full = np.full((th, tw), 255, np.uint8)  # saturated frame, saturated template
            rc, num, w2 = ctx.match_template(2, full)
            assert rc == OK and np.all(num == 255 * 255 * tw * th) and np.all(w2 == 255 * 255 * tw * th), (tw, th)
        assert ctx.match_template(0, np.ones((1, W + 1), np.uint8))[0] == E_INVALID  # tw > W
        assert ctx.match_template(0, np.ones((H + 1, 1), np.uint8))[0] == E_INVALID  # th > H
        assert ctx.match_template(3, np.ones((1, 1), np.uint8))[0] == E_INVALID      # no such frame
        assert ctx.match_template(-1, np.ones((1, 1), np.uint8))[0] == E_INVALID


# ------------------------------------------------------------------------------------------------------------------
# full size
# ------------------------------------------------------------------------------------------------------------------
def test_full_size_frame_calls(oracle):
    W, H, F = 1680, 1050, 3
    ctx, fr, mu, sigma = loaded(W, H, F, 1680)
    roi = (100, 300, 200, 500)  # the size of a bellows region of the camera masks
    with ctx:
        D = nonzero(oracle.process_frame(fr[2], fr[0], sigma))
        rc, Dg, hg = ctx.diff_frame(2, 0)
        assert rc == OK and np.array_equal(Dg, D) and np.array_equal(hg, oracle.hist256(D))
        check_current(ctx, D, thr=3)
        for a, b in ((0, 2), (2, 0)):
            R = nonzero(oracle.process_frame(fr[a], fr[b], sigma, roi=roi))
            rc, Rg, hg = ctx.diff_frame_roi(a, b, roi)
            assert rc == OK and np.array_equal(Rg, R) and np.array_equal(hg, oracle.hist256(R)), (a, b)
        check_current(ctx, R)
        O = nonzero(oracle.posttrig_frame(fr[2], mu, sigma))
        rc, Og, hg = ctx.posttrig(2)
        assert rc == OK and np.array_equal(Og, O) and np.array_equal(hg, oracle.hist256(O))
        check_current(ctx, O, thr=-1)  # all 1.76 M pixels through abub_ctx_foreground
        rc, h = ctx.batch(2, 0, F)
        assert rc == OK and np.array_equal(h[2], oracle.hist256(D))


# ------------------------------------------------------------------------------------------------------------------
# independence and lifecycle
# ------------------------------------------------------------------------------------------------------------------
def run_sequence(ctx, job):
    """set_model -> upload -> batch -> diff_frame -> posttrig -> foreground for every stack of the job; returns the
    first mismatch as text, or None."""
    for s, st in enumerate(job["stacks"]):
        if ctx.set_model(st["mu"], st["sigma"]) != OK or ctx.upload(list(st["fr"])) != OK:
            return "stack %d: set_model / upload" % s
        F = len(st["fr"])
        rc, h = ctx.batch(2, 1, F - 1)
        if rc != OK or not np.array_equal(h, st["hists"]):
            return "stack %d: batch" % s
        rc, D, h = ctx.diff_frame(F - 1, 0)
        if rc != OK or not np.array_equal(D, st["D"]) or not np.array_equal(h, st["hD"]):
            return "stack %d: diff_frame" % s
        rc, n, idx = ctx.foreground(2, D.size)
        if rc != OK or not np.array_equal(np.sort(idx[:n]), st["fgD"]):
            return "stack %d: foreground of D" % s
        rc, O, h = ctx.posttrig(F - 1)
        if rc != OK or not np.array_equal(O, st["O"]) or not np.array_equal(h, st["hO"]):
            return "stack %d: posttrig" % s
        rc, n, idx = ctx.foreground(5, O.size)
        if rc != OK or not np.array_equal(np.sort(idx[:n]), st["fgO"]):
            return "stack %d: foreground of O" % s
    return None


def make_job(oracle, W, H, nstacks, F, seed):
    stacks = []
    for s in range(nstacks):
        fr, base = make_stack(W, H, F, seed + 100 * s)
        mu, sigma = make_model(W, H, base, seed + 100 * s, saturated=(s % 2 == 1))
        D = nonzero(oracle.process_frame(fr[F - 1], fr[0], sigma))
        O = nonzero(oracle.posttrig_frame(fr[F - 1], mu, sigma))
        hists = np.stack([oracle.hist256(nonzero(oracle.process_frame(fr[i], fr[max(i - 2, 0)], sigma)))
                          for i in range(1, F)])
        stacks.append(dict(fr=fr, mu=mu, sigma=sigma, D=D, hD=oracle.hist256(D), O=O, hO=oracle.hist256(O), hists=hists,
                           fgD=np.flatnonzero(D.ravel() > 2), fgO=np.flatnonzero(O.ravel() > 5)))
    return dict(W=W, H=H, F=F, stacks=stacks)


def test_four_contexts_in_four_threads(oracle):
    F = 6
    jobs = [make_job(oracle, W, H, 6, F, 1000 * k) for k, (W, H) in enumerate(((1280, 64), (1680, 50), (322, 37), (268, 20)))]
    ctxs = [Ctx(j["W"], j["H"], F) for j in jobs]
    barrier = threading.Barrier(len(jobs))
    results = [None] * len(jobs)

    def work(k):
        try:
            barrier.wait(timeout=60)
            for _ in range(3):
                bad = run_sequence(ctxs[k], jobs[k])
                if bad:
                    results[k] = bad
                    return
            results[k] = "ok"
        except Exception as e:  # noqa: BLE001  (reported through the result list)
            results[k] = repr(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(jobs))]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        assert not any(t.is_alive() for t in threads)
    finally:
        for c in ctxs:
            c.close()
    assert results == ["ok"] * len(jobs), results


def test_two_contexts_used_alternately(oracle):
    W, H, F = 1280, 64, 4
    ja = make_job(oracle, W, H, 1, F, 41)["stacks"][0]
    jb = make_job(oracle, W, H, 1, F, 42)["stacks"][0]
    assert not np.array_equal(ja["D"], jb["D"]) and not np.array_equal(ja["O"], jb["O"])
    with Ctx(W, H, F) as a, Ctx(W, H, F) as b:
        for c, j in ((a, ja), (b, jb)):
            assert c.set_model(j["mu"], j["sigma"]) == OK and c.upload(list(j["fr"])) == OK
        for _ in range(2):
            for (c, j), (o, oj) in (((a, ja), (b, jb)), ((b, jb), (a, ja))):
                rc, D, h = c.diff_frame(F - 1, 0)
                assert rc == OK and np.array_equal(D, j["D"]) and np.array_equal(h, j["hD"])
                rc, O, h = o.posttrig(F - 1)  # the other context works in between
                assert rc == OK and np.array_equal(O, oj["O"]) and np.array_equal(h, oj["hO"])
                check_current(c, j["D"], thr=2)
                check_current(o, oj["O"], thr=5)
                rc, h = c.batch(2, 1, F - 1)
                assert rc == OK and np.array_equal(h, j["hists"])


def test_create_use_destroy_twenty_times(oracle):
    W, H, F = 1680, 50, 4
    job = make_job(oracle, W, H, 1, F, 77)
    L = _lib.lib()
    L.abub_ctx_destroy(None)  # a no-op
    for round_ in range(20):
        with Ctx(W, H, F) as ctx:
            assert run_sequence(ctx, job) is None, round_
        L.abub_ctx_destroy(None)
