"""K4b (abub_label_blobs_dev, abub_blobs.hip) where its five older tests do not go: foreground counts on both sides of the
2048-pixel limit between the LDS path and the dense-plane path, workgroups of the dense-plane path that take a second and
a third slot on the same planes, launches of more than 1024 slots (several slots per thread in the offset scan), the
comp = NULL form the pipeline uses, shapes that use one neighbour relation at a time or wrap around the raster, the
equalities of the two comparisons, and the pipeline's call sequence at the benchmark's slot count.

Every comparison is exact, against blobscenes._reference (scipy.ndimage.label, 3 x 3 structure; pinned on the CPU by
test_blob_scenes.py).  Every launch asserts stats[0], the number of slots labelled on the dense planes: a case meant for
one path must not quietly run on the other."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import blobscenes as bs  # noqa: E402
from autobub3hs_amd import _lib, hip, host  # noqa: E402
from blobscenes import DEV, LDS_N, _assert_same_outputs, _check, _reference, _slot_image  # noqa: E402

CANARY = -7
GUARD = 4096
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)


def _list(imgs, rs, order="shuffled", cands=None):
    """grouped candidate list: per slot contiguous, inside a slot in raster order ("sorted"), backwards ("reversed") or
    shuffled with rs.  A slot's candidates are its pixels with value > 0, or cands[s] (bool image) where that is given:
    a list may hold value-0 pixels."""
    offs, idx, val = [0], [], []
    for s, v in enumerate(imgs):
        c = v > 0 if cands is None or cands[s] is None else cands[s]
        i = np.flatnonzero(c.ravel()).astype(np.int64)
        if order == "reversed":
            i = i[::-1]
        elif order == "shuffled":
            rs.shuffle(i)
        else:
            assert order == "sorted"
        idx.append(i)
        val.append(v.ravel()[i])
        offs.append(offs[-1] + len(i))
    return np.array(offs, np.int64), np.concatenate(idx + [np.zeros(1, np.int64)]), np.concatenate(val + [np.zeros(1, np.uint8)])


def _run(lst, thr, mb, W, H, **kw):
    offs, idx, val = lst
    out = hip.label_blobs(_t(offs, np.int32), _t(idx, np.int32), _t(val, np.uint8), _t(thr, np.int32), _t(mb, np.int32), W, H,
                          **kw)
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    assert out["kept_off"][0] == 0 and out["comp_off"][0] == 0
    return out


def _nlarge(imgs, thr):
    return sum(int((v > t).sum()) > LDS_N for v, t in zip(imgs, thr))


def _descs(out, s):
    co = out["comp_off"]
    return [tuple(int(x) for x in r) for r in out["comp"][co[s]:co[s + 1]]]


def _assert_counts(names, out, want):
    """ncomp of every named slot at once, so that a failure names every shape that is wrong, not only the first"""
    got = [int(c) for c in out["ncomp"][:len(names)]]
    assert got == list(want), {nm: (g, w) for nm, g, w in zip(names, got, want) if g != w}


def _same_but_descriptors(out, out2):
    """a comp = NULL launch against a launch with descriptors of the same list"""
    assert out2["comp"] is None
    _assert_same_outputs({k: v for k, v in out.items() if k != "comp"}, {k: v for k, v in out2.items() if k != "comp"})


# ---- a. the path limit ---------------------------------------------------------------------------------------------------

LIMIT_N = [1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 2050]


@pytest.mark.parametrize("blob", ["lattice", "compact"])
@pytest.mark.parametrize("W,H", [(1680, 1050), (322, 37)])
def test_path_limit(W, H, blob):
    """slots of exactly n foreground pixels around the bitonic padding steps (1, 2, 1024, 1025) and the LDS limit (2047,
    2048 = the LDS arrays filled to the last position, 2049, 2050), as n isolated pixels and as one compact blob (real
    unions at n = 2048); an empty slot; and a slot of 5000 candidates of which exactly 2048 lie above thr: the foreground
    count chooses the path, not the candidate count"""
    rs = np.random.RandomState(W + len(blob))
    if blob == "lattice":
        imgs = [bs.lattice(H, W, n, seed=n) for n in LIMIT_N]
        body = bs.lattice(H, W, 2048, seed=77)
    else:
        imgs = [bs.compact(H, W, n, x=(7 * k) % 40, y=0) for k, n in enumerate(LIMIT_N)]
        body = bs.compact(H, W, 2048, x=W - 60, y=0)
    imgs.append(np.zeros((H, W), np.uint8))
    # 2048 pixels of value 101 .. 255 and 2952 more candidates of value 1 .. 100, anywhere (next to the others too)
    body = np.where(body > 0, 101 + body % 155, 0).astype(np.uint8)
    rest = rs.choice(np.flatnonzero(body.ravel() == 0), 5000 - 2048, replace=False)
    body.ravel()[rest] = rs.randint(1, 101, len(rest))
    assert (body > 0).sum() == 5000 and (body > 100).sum() == 2048
    imgs.append(body)
    thr = np.array([0] * (len(LIMIT_N) + 1) + [100])
    mb = np.array([[-1, 0, 10][k % 3] for k in range(len(imgs))])
    for n, v in zip(LIMIT_N, imgs):
        assert (v > 0).sum() == n
    out = _run(_list(imgs, rs), thr, mb, W, H)
    st = _check(imgs, thr, mb, out)
    assert st[0] == sum(n > LDS_N for n in LIMIT_N) == 2  # 2049 and 2050 only: the 5000-candidate slot stays in LDS
    for s, n in enumerate(LIMIT_N):
        if blob == "lattice":  # isolated pixels: 10 keeps nothing, 0 and -1 keep everything
            want = 0 if mb[s] == 10 else n
            assert out["ncomp"][s] == n and out["nkept_comp"][s] == want
            assert out["kept_off"][s + 1] - out["kept_off"][s] == want
        else:
            assert out["ncomp"][s] == 1
    out2 = _run(_list(imgs, rs), thr, mb, W, H, comp=False)
    _same_but_descriptors(out, out2)


# ---- b. plane reuse --------------------------------------------------------------------------------------------------------

def _raw_launch(lst, thr, mb, W, H, scratch, in_cap=None, comp=True):
    """abub_label_blobs_dev on a scratch buffer of the caller's, with cap = in_cap and canaries behind kept_idx / comp"""
    offs, idx, val = lst
    n = len(thr)
    in_cap = len(idx) if in_cap is None else in_cap
    cap = in_cap
    L = _lib.lib()
    need = L.abub_label_blobs_scratch_bytes(n, W, H, in_cap, 1 if comp else 0)
    assert 0 < need <= scratch.numel()
    d = [_t(offs, np.int32), _t(idx, np.int32), _t(val, np.uint8), _t(thr, np.int32), _t(mb, np.int32)]
    kidx = torch.full((cap + GUARD,), CANARY, dtype=torch.int32, device=DEV)
    cbuf = torch.full((cap + GUARD, 6), CANARY, dtype=torch.int32, device=DEV)
    ko, nc, nk, co, stats = (torch.full((m,), CANARY, dtype=torch.int32, device=DEV) for m in (n + 1, n, n, n + 1, 4))
    rc = L.abub_label_blobs_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), in_cap, n, W, H, d[3].data_ptr(),
                                d[4].data_ptr(), ko.data_ptr(), kidx.data_ptr(), cap, nc.data_ptr(), nk.data_ptr(),
                                co.data_ptr(), cbuf.data_ptr() if comp else None, cap if comp else 0, stats.data_ptr(),
                                scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "abub_label_blobs_dev")
    torch.cuda.synchronize()
    k, c = kidx.cpu().numpy(), cbuf.cpu().numpy()
    assert (k[cap:] == CANARY).all() and (c[cap:] == CANARY).all()  # nothing at or past cap
    if not comp:
        assert (c == CANARY).all()
    return {"kept_off": ko.cpu().numpy(), "kept_idx": k[:cap], "ncomp": nc.cpu().numpy(), "nkept_comp": nk.cpu().numpy(),
            "comp_off": co.cpu().numpy(), "comp": c[:cap] if comp else None, "stats": stats.cpu().numpy()}


def _reuse_scene(W, H):
    """13 large slots for the 4 workgroups of the dense-plane path (one takes four, three take three), small and empty ones
    in between.  The large ones alternate between complementary patterns: v on a 35 % random mask and on that mask's
    complement, the checkerboard and its inverse; every random mask is drawn afresh, so whichever slot a workgroup had
    before on its planes (the order of the large-slot list depends on the launch), the next one's foreground covers
    pixels that were background there and the other way round."""
    rs = np.random.RandomState(96)
    chk = bs.checkerboard(H, W) > 0
    imgs, thr = [], []
    for k in range(13):
        kind = k % 4
        if kind in (0, 1):
            m = rs.rand(H, W) < 0.35
            if kind == 1:
                m = ~m
        else:
            m = chk if kind == 2 else ~chk
        v = np.zeros((H, W), np.uint8)
        v[m] = rs.randint(1, 256, int(m.sum()))
        imgs.append(v)
        thr.append(0 if k % 3 else 20)
        imgs.append(_slot_image(rs, W, H, "small" if k % 2 else "empty"))
        thr.append(int(rs.randint(0, 100)))
    thr = np.array(thr)
    mb = np.array([[-1, 10, 0][s % 3] for s in range(len(imgs))])
    return imgs, thr, mb, rs


def test_plane_reuse():
    """the workgroups of k4b_large loop over more slots than there are workgroups: each must leave its label plane zero for
    its next slot (a ghost of the slot before would join or add pixels), also across launches on one scratch buffer that
    the caller never clears, and after a launch whose list had overflowed"""
    W, H = 1280, 96
    imgs, thr, mb, rs = _reuse_scene(W, H)
    nl = _nlarge(imgs, thr)
    assert nl == 13
    lst = _list(imgs, rs)
    L = _lib.lib()
    need = L.abub_label_blobs_scratch_bytes(len(imgs), W, H, len(lst[1]), 1)
    scratch = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)  # the header asks for no particular content
    out = _raw_launch(lst, thr, mb, W, H, scratch)
    assert _check(imgs, thr, mb, out)[0] == nl
    # again on the same scratch, slots in reverse order: slot s is now slot n-1-s, with the same result
    r_imgs, r_thr, r_mb = imgs[::-1], thr[::-1].copy(), mb[::-1].copy()
    out_r = _raw_launch(_list(r_imgs, rs), r_thr, r_mb, W, H, scratch)
    assert _check(r_imgs, r_thr, r_mb, out_r)[0] == nl
    n = len(imgs)
    for s in range(n):
        a, b = out["kept_off"], out_r["kept_off"]
        assert np.array_equal(out["kept_idx"][a[s]:a[s + 1]], out_r["kept_idx"][b[n - 1 - s]:b[n - s]]), s
        assert _descs(out, s) == _descs(out_r, n - 1 - s), s
    # an overflowed producer list: offsets are true counts and run past in_cap.  The header promises only that nothing is
    # read at or past in_cap or written at or past cap, and no error
    in_cap = int(lst[0][8]) + 1000  # inside the fifth large slot
    assert lst[0][8] < in_cap < lst[0][9] < len(lst[1])
    _raw_launch(lst, thr, mb, W, H, scratch, in_cap=in_cap)
    # the full list again, same scratch: exact
    out2 = _raw_launch(lst, thr, mb, W, H, scratch)
    assert _check(imgs, thr, mb, out2)[0] == nl
    _assert_same_outputs(out, out2)
    out3 = _raw_launch(lst, thr, mb, W, H, scratch, comp=False)
    _check(imgs, thr, mb, out3)
    _same_but_descriptors(out, out3)


# ---- c. slot counts ---------------------------------------------------------------------------------------------------------

_SLOTS = {}


def _many_slots(n, W, H):
    """n seeded slots (every 7th empty, every 500th large) and their references, built once for the largest n"""
    if not _SLOTS:
        rs = np.random.RandomState(4097)
        nmax = 4097
        kinds = ["large" if s % 500 == 499 else "empty" if s % 7 == 6 else "small" for s in range(nmax)]
        imgs = [_slot_image(rs, W, H, k) for k in kinds]
        thr = rs.randint(0, 120, nmax)
        thr[499::500] = 0
        mb = np.array([[-1, 0, 10][s % 3] for s in range(nmax)])
        _SLOTS["v"] = (imgs, thr, mb, [_reference(imgs[s], thr[s], mb[s]) for s in range(nmax)])
    imgs, thr, mb, refs = _SLOTS["v"]
    return imgs[:n], thr[:n], mb[:n], refs[:n]


@pytest.mark.parametrize("nslots", [1024, 1025, 2200, 4097])
def test_slot_counts(nslots):
    """k4b_scan is one block of 1024 threads: above 1024 slots every thread scans several (the benchmark shape launches
    about 2200 with the blobs knob on).  kept_off / comp_off == cumsum of the reference counts, every slot's content ==
    the reference, with descriptors and without."""
    W, H = 160, 64
    imgs, thr, mb, refs = _many_slots(nslots, W, H)
    rs = np.random.RandomState(nslots)
    nfg = np.array([int((v > t).sum()) for v, t in zip(imgs, thr)])
    nl = int((nfg > LDS_N).sum())
    assert nl >= nslots // 500 >= 2
    want_ko = np.concatenate([[0], np.cumsum([len(r[2]) for r in refs])])
    want_co = np.concatenate([[0], np.cumsum([len(r[1]) for r in refs])])
    want_kept = np.concatenate([r[2] for r in refs])
    want_comp = np.array([c for r in refs for c in r[1]], np.int64).reshape(-1, 6)
    lst = _list(imgs, rs)
    for comp in (True, False):
        out = _run(lst, thr, mb, W, H, comp=comp)
        assert np.array_equal(out["kept_off"], want_ko)
        assert np.array_equal(out["comp_off"], want_co)
        assert np.array_equal(out["ncomp"], [r[0] for r in refs])
        assert np.array_equal(out["nkept_comp"], np.diff(want_co))
        bad = [s for s in range(nslots) if not np.array_equal(out["kept_idx"][want_ko[s]:want_ko[s + 1]], refs[s][2])]
        assert not bad, bad[:10]
        assert np.array_equal(out["kept_idx"][:want_ko[-1]], want_kept)
        if comp:
            assert np.array_equal(out["comp"][:want_co[-1]], want_comp)
        assert list(out["stats"]) == [nl, nfg.sum(), sum(r[0] for r in refs), want_co[-1]]


# ---- d. shapes, on both paths ---------------------------------------------------------------------------------------------

def _lds_scene(name, H, W):
    """the shape for the LDS path: as it is where it has at most 2048 pixels, else cropped: generated for the widest
    frame (H, w) that stays within 2048 pixels and pasted against the right border of the (H, W) frame, so the row pitch
    is still W and the shape still touches the top, bottom and right borders -> (image, components)"""
    gen, count, _ = bs.SHAPES[name]
    w = W
    while (gen(H, w) > 0).sum() > LDS_N:
        w -= 1
    v = np.zeros((H, W), np.uint8)
    v[:, W - w:] = gen(H, w)
    return v, count(H, w)


def _dense_scene(name, H, W, seed):
    """the shape for the dense-plane path: as it is where it has more than 2048 pixels, else in one slot with a
    lattice(2049) that keeps two pixels away from it -> (image, components)"""
    gen, count, _ = bs.SHAPES[name]
    v = gen(H, W)
    if (v > 0).sum() > LDS_N:
        return v, count(H, W)
    return np.maximum(v, bs.lattice(H, W, LDS_N + 1, seed=seed, avoid=v)), count(H, W) + LDS_N + 1


def _ring_descs(H, W, x_off=0):
    return [(y0 * W + x0 + x_off, x0 + x_off, y0, x1 + x_off, y1, 2 * (x1 - x0 + 1) + 2 * (y1 - y0 + 1) - 4)
            for x0, y0, x1, y1 in bs.ring_boxes(H, W - x_off)]


def _wrap_descs(W):
    return [(W - 1, W - 1, 0, W - 1, 0, 1), (W, 0, 1, 0, 1, 1)]


@pytest.mark.parametrize("H,W", [(24, 40), (37, 322)])
def test_shapes_lds_path(H, W):
    """every generator as a slot of at most 2048 foreground pixels (cropped as _lds_scene says where the frame holds
    more), min box -1 and 10, with descriptors and without"""
    names = list(bs.SHAPES)
    scenes = [_lds_scene(nm, H, W) for nm in names]
    imgs = [v for v, _ in scenes]
    n = len(imgs)
    thr = np.zeros(n, np.int64)
    rs = np.random.RandomState(H)
    assert all(0 < (v > 0).sum() <= LDS_N for v in imgs)
    outs = {}
    for m in (-1, 10):
        mb = np.full(n, m)
        out = outs[m] = _run(_list(imgs, rs), thr, mb, W, H)
        _assert_counts(names, out, [c for _, c in scenes])
        assert _check(imgs, thr, mb, out)[0] == 0
    out = outs[-1]
    s = names.index("rings")
    w = int((imgs[s] > 0).any(axis=0).sum())
    assert _descs(out, s) == _ring_descs(H, W, W - w) and len(_descs(out, s)) > 1  # every ring apart, box = its rectangle
    assert _descs(out, names.index("wrap_pair")) == _wrap_descs(W)  # two components of one pixel each
    assert outs[10]["nkept_comp"][names.index("wrap_pair")] == 0
    out2 = _run(_list(imgs, rs), thr, np.full(n, 10), W, H, comp=False)
    _check(imgs, thr, np.full(n, 10), out2)
    _same_but_descriptors(outs[10], out2)


@pytest.mark.parametrize("H,W", [(1050, 1680), (1024, 1280)])
def test_shapes_dense_planes(H, W):
    """every generator as a slot of more than 2048 foreground pixels, under three list orders: byte-identical outputs
    ("Exact and deterministic")"""
    names = list(bs.SHAPES)
    scenes = [_dense_scene(nm, H, W, seed=k) for k, nm in enumerate(names)]
    imgs = [v for v, _ in scenes]
    n = len(imgs)
    thr = np.zeros(n, np.int64)
    rs = np.random.RandomState(W)
    assert _nlarge(imgs, thr) == n
    keep_all, mb10 = np.full(n, -1), np.full(n, 10)
    out = _run(_list(imgs, rs, "sorted"), thr, keep_all, W, H)
    _assert_counts(names, out, [c for _, c in scenes])
    assert _check(imgs, thr, keep_all, out)[0] == n
    assert _descs(out, names.index("rings")) == _ring_descs(H, W)
    assert [d for d in _descs(out, names.index("wrap_pair")) if d[0] in (W - 1, W)] == _wrap_descs(W)
    out_r = _run(_list(imgs, rs, "reversed"), thr, keep_all, W, H)
    _assert_same_outputs(out, out_r)
    del out_r
    out_s = _run(_list(imgs, rs, "shuffled"), thr, keep_all, W, H)
    _assert_same_outputs(out, out_s)
    del out, out_s
    out10 = _run(_list(imgs, rs, "shuffled"), thr, mb10, W, H)
    assert _check(imgs, thr, mb10, out10)[0] == n
    out_n = _run(_list(imgs, rs, "shuffled"), thr, mb10, W, H, comp=False)
    assert out_n["stats"][0] == n
    _same_but_descriptors(out10, out_n)


@pytest.mark.parametrize("H,W", [(17, 1), (17, 2), (17, 3), (1, 17), (2, 17), (1, 1), (2, 2),
                                 (3000, 1), (3000, 2), (3000, 3), (1, 3000), (2, 3000)])
def test_shapes_on_frames_one_to_three_pixels_wide_or_high(H, W):
    """W in {1, 2, 3} and H in {1, 2}: every neighbour test sits on a border.  The short frames run on the LDS path; on the
    3000-pixel frames the full lines, stripes and snakes exceed 2048 pixels and run on the dense planes."""
    names = list(bs.SHAPES)
    imgs = [bs.SHAPES[nm][0](H, W) for nm in names]
    if bs.lattice_capacity(H, W) >= 5:
        imgs.append(bs.lattice(H, W, min(bs.lattice_capacity(H, W), LDS_N), seed=H))
    n = len(imgs)
    thr = np.zeros(n, np.int64)
    rs = np.random.RandomState(H + W)
    nl = _nlarge(imgs, thr)
    assert (nl > 0) == (H * W >= 3000)
    for m, comp in ((-1, True), (10, True), (10, False)):
        mb = np.full(n, m)
        out = _run(_list(imgs, rs), thr, mb, W, H, comp=comp)
        _assert_counts(names, out, [bs.SHAPES[nm][1](H, W) for nm in names])
        assert _check(imgs, thr, mb, out)[0] == nl


# ---- e. equalities -----------------------------------------------------------------------------------------------------------

E_MB = [9, 10, 11, INT32_MAX, 0, -1]
E_KEPT = [2, 1, 0, 0, 2, 2]  # of the 5 x 2 box (area 10) and the 11 x 1 box (area 11): kept iff area > min_box_area


def _two_boxes(H, W):
    v = np.zeros((H, W), np.uint8)
    v[3:5, 4:9] = 90      # 5 x 2
    v[H - 1, W - 11:] = 80  # 11 x 1, in the last row up to the last pixel
    return v


@pytest.mark.parametrize("dense", [False, True])
def test_equalities(dense):
    """bbox area == min_box_area is dropped and area == min_box_area + 1 is kept, up to INT32_MAX; val == thr is background
    and val == thr + 1 foreground; thr = 255 leaves a slot empty; thr = -1 makes the value-0 candidates of a list
    foreground (a K4 list made with a negative threshold holds them)"""
    H, W = 37, 322
    rs = np.random.RandomState(int(dense))

    def slot(v, seed, n=LDS_N + 1, avoid=None):
        """dense: the same scene in one slot with n isolated pixels, two pixels away from it"""
        if not dense:
            return v
        return np.maximum(v, bs.lattice(H, W, n, seed=seed, avoid=(v > 0) if avoid is None else avoid))

    imgs = [slot(_two_boxes(H, W), k) for k in range(len(E_MB))]
    thr, mb = [0] * len(E_MB), list(E_MB)
    # val == thr / thr + 1: two 5 x 2 boxes side by side, values 100 and 101, thr 100 -> one 5 x 2 component; the
    # isolated pixels straddle thr as well (four in five stay: still above the LDS limit)
    v = np.zeros((H, W), np.uint8)
    v[10:12, 20:25], v[10:12, 25:30] = 100, 101
    lat = slot(np.zeros((H, W), np.uint8), 10, n=2900, avoid=v > 0)
    imgs.append(np.where(lat > 0, 100 + (lat % 5 > 0), v).astype(np.uint8))
    thr.append(100)
    mb.append(9)
    # thr = 255: nothing, although the slot has candidates of value 255
    imgs.append(slot(np.where(_two_boxes(H, W) > 0, 255, 0).astype(np.uint8), 11))
    thr.append(255)
    mb.append(-1)
    # thr = -1: candidates of value 0 are foreground; the pixels outside the list are not
    v = _two_boxes(H, W)
    zero = np.zeros((H, W), bool)
    zero[3:5, 9:12] = True  # value-0 candidates that widen the 5 x 2 box to 8 x 2
    zero[20, 30] = True     # and one on its own
    imgs.append(slot(v, 12, avoid=(v > 0) | zero))
    cand = (imgs[-1] > 0) | zero
    thr.append(-1)
    mb.append(15)
    cands = [None] * (len(imgs) - 1) + [cand]
    thr, mb = np.array(thr), np.array(mb)
    # what the reference sees: the list's pixels with their values, every other pixel below any threshold
    ref_imgs = [np.where(v > 0 if c is None else c, v.astype(np.int16), -2) for v, c in zip(imgs, cands)]
    out = _run(_list(imgs, rs, cands=cands), thr, mb, W, H)
    st = _check(ref_imgs, thr, mb, out)
    nfg = [int((r > t).sum()) for r, t in zip(ref_imgs, thr)]
    assert st[0] == sum(f > LDS_N for f in nfg) == (len(imgs) - 1 if dense else 0)
    box52, box111 = (3 * W + 4, 4, 3, 8, 4, 10), ((H - 1) * W + W - 11, W - 11, H - 1, W - 1, H - 1, 11)
    for s, m in enumerate(E_MB):
        got = [d for d in _descs(out, s) if d[5] > 1]
        assert got == [box52, box111][2 - E_KEPT[s]:], (m, got)
        assert out["ncomp"][s] == 2 + (LDS_N + 1 if dense else 0)
        assert out["nkept_comp"][s] == E_KEPT[s] + (LDS_N + 1 if dense and m in (0, -1) else 0)
    s = len(E_MB)
    assert [d for d in _descs(out, s) if d[5] > 1] == [(10 * W + 25, 25, 10, 29, 11, 10)]
    s += 1
    assert out["ncomp"][s] == out["nkept_comp"][s] == 0
    assert out["kept_off"][s] == out["kept_off"][s + 1] and out["comp_off"][s] == out["comp_off"][s + 1]
    s += 1
    assert [d for d in _descs(out, s) if d[5] > 1] == [(3 * W + 4, 4, 3, 11, 4, 16)]  # 8 x 2 > 15; 11 x 1 and 1 x 1 dropped
    assert out["ncomp"][s] == 3 + (LDS_N + 1 if dense else 0)
    out2 = _run(_list(imgs, rs, cands=cands), thr, mb, W, H, comp=False)
    _same_but_descriptors(out, out2)


# ---- f. the pipeline's call sequence at the benchmark's slot count -------------------------------------------------------

def test_production_chain_2200_images():
    """K4 pairs with the per-image TOZERO cut -> group by slot -> device Otsu on the images' histograms -> K4b with
    comp = NULL, min box 10 (tracking images) / -1 (genesis images): the calls the batched pipeline makes for widths off
    the fast path, at the slot count of the benchmark shape with the blobs knob on.  Per image: threshold ==
    host.binarize_threshold, kept pixels == the reference's."""
    W, H, n = 160, 64, 2200
    P = W * H
    rs = np.random.RandomState(2200)
    img = np.zeros((n, H, W), np.uint8)
    noise = rs.rand(n, H, W) < 0.03
    img[noise] = rs.randint(1, 40, int(noise.sum()))
    yy, xx = np.mgrid[0:H, 0:W]
    for s in range(n):
        for _ in range(rs.randint(0, 4)):  # bubbles: discs of radius 1 .. 9, some over the border
            cy, cx, r = rs.randint(-3, H + 3), rs.randint(-3, W + 3), rs.randint(1, 10)
            d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
            img[s][d] = np.maximum(img[s][d], rs.randint(60, 256, int(d.sum())))
    img[7] = 0                                                     # a blank image
    img[11] = np.maximum(img[11], rs.randint(0, 2, (H, W)) * 200)  # a dense one: above the LDS limit
    tozero = rs.choice([3, 5, 10, 30], n).astype(np.int32)
    mb = np.where(np.arange(n) % 11 == 0, -1, 10).astype(np.int32)
    hist = np.stack([np.bincount(im.ravel(), minlength=256) for im in img])
    total = int((img > tozero[:, None, None]).sum())
    cap = total + 64
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    d_img, d_tz = torch.from_numpy(img).to(DEV), torch.from_numpy(tozero).to(DEV)
    pairs = torch.empty((cap, 2), dtype=torch.int32, device=DEV)
    count = torch.zeros((1,), dtype=torch.int32, device=DEV)
    _lib.check(L.abub_fg_compact_pairs_dev(d_img.data_ptr(), n, W, H, d_tz.data_ptr(), pairs.data_ptr(), cap, count.data_ptr(),
                                           st), "abub_fg_compact_pairs_dev")
    gscratch = torch.zeros((2 * n,), dtype=torch.int32, device=DEV)
    offs = torch.empty((n + 1,), dtype=torch.int32, device=DEV)
    idx = torch.empty((cap,), dtype=torch.int32, device=DEV)
    val = torch.empty((cap,), dtype=torch.uint8, device=DEV)
    _lib.check(L.abub_pairs_group_dev(pairs.data_ptr(), count.data_ptr(), cap, n, gscratch.data_ptr(), offs.data_ptr(),
                                      idx.data_ptr(), val.data_ptr(), st), "abub_pairs_group_dev")
    otsu = hip.binarize_thr(_t(hist, np.int32), d_tz, W, H)
    out = hip.label_blobs(offs, idx, val, otsu, torch.from_numpy(mb).to(DEV), W, H, comp=False)
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    assert int(count.item()) == total == int(offs[-1].item())
    thr = otsu.cpu().numpy()
    want = np.array([host.binarize_threshold(hist[s], P, tozero[s]) for s in range(n)])
    assert np.array_equal(thr, want)
    assert (thr >= tozero).all()  # every foreground pixel is in the list
    st_ = _check(list(img), want, mb, out)
    assert st_[0] == _nlarge(img, want) >= 1
    assert out["ncomp"][7] == 0 and out["kept_off"][7] == out["kept_off"][8]
