"""K4b (abub_label_blobs_dev) test scenes: the slot images, the grouped candidate list, the scipy reference and the launch /
check helpers of test_gpu_blobs.py and test_gpu_blobs_limits.py, and shape generators (H, W, ...) -> u8 image whose
8-connected component count is stated next to them (SHAPES, checked on the CPU by test_blob_scenes.py).

Not collected by pytest.  Nothing here needs a GPU until _launch() is called."""
import numpy as np

try:
    import torch
except ImportError:  # the generators and the reference work without it
    torch = None

DEV = "cuda:0"
LDS_N = 2048  # abub_blobs.hip K4B_LDS_N: a slot with more foreground pixels is labelled on the dense planes
FG = 200      # value of a generated shape's foreground pixels


def _slot_image(rs, W, H, kind):
    """-> values u8 [H, W]; the candidate list of a slot is every pixel with value > 0"""
    v = np.zeros((H, W), np.uint8)
    if kind == "empty":
        return v
    if kind == "large":  # >= 200k foreground pixels: the global-memory path
        m = rs.rand(H, W) < 0.35
        v[m] = rs.randint(1, 256, m.sum())
        return v
    n = rs.randint(1, 1500)
    ys, xs = rs.randint(0, H, n), rs.randint(0, W, n)
    v[ys, xs] = rs.randint(1, 256, n)
    for _ in range(rs.randint(0, 6)):  # a few blobs, some on the edges
        h, w = rs.randint(1, 12), rs.randint(1, 12)
        y, x = rs.randint(-3, H), rs.randint(-3, W)
        y0, y1, x0, x1 = max(y, 0), min(y + h, H), max(x, 0), min(x + w, W)
        if y1 > y0 and x1 > x0:
            v[y0:y1, x0:x1] = np.maximum(v[y0:y1, x0:x1], rs.randint(100, 256, (y1 - y0, x1 - x0)).astype(np.uint8))
    return v


def _grouped(imgs, rs):
    """grouped candidate list as abub_pairs_group_*_dev leave it: per slot contiguous, unordered inside the slot"""
    offs, idx, val = [0], [], []
    for v in imgs:
        i = np.flatnonzero(v.ravel()).astype(np.int64)
        rs.shuffle(i)
        idx.append(i)
        val.append(v.ravel()[i])
        offs.append(offs[-1] + len(i))
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    val = np.concatenate(val) if val else np.zeros(0, np.uint8)
    return np.array(offs, np.int64), idx, val


def _reference(v, thr, mb):
    from scipy import ndimage

    m = v > thr
    lab, n = ndimage.label(m, structure=np.ones((3, 3)))
    comps = []
    keep = np.zeros(n + 1, bool)
    first = ndimage.minimum(np.arange(v.size).reshape(v.shape), lab, np.arange(1, n + 1)) if n else []
    counts = np.bincount(lab.ravel(), minlength=n + 1)
    for k, sl in enumerate(ndimage.find_objects(lab), start=1):
        y0, y1, x0, x1 = sl[0].start, sl[0].stop - 1, sl[1].start, sl[1].stop - 1
        keep[k] = mb < 0 or (x1 - x0 + 1) * (y1 - y0 + 1) > mb
        if keep[k]:
            comps.append((int(first[k - 1]), x0, y0, x1, y1, int(counts[k])))
    comps.sort()
    kept = np.flatnonzero(keep[lab].ravel() & m.ravel())
    return n, comps, kept


def _launch(imgs, thr, mb, W, H, rs, **kw):
    """comp=False (handed on to hip.label_blobs) is the pipeline's form: comp = NULL, scratch without descriptors"""
    from autobub3hs_amd import hip

    offs, idx, val = _grouped(imgs, rs)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)  # noqa: E731
    out = hip.label_blobs(t(offs, np.int32), t(np.concatenate([idx, [0]]), np.int32), t(np.concatenate([val, [0]]), np.uint8),
                          t(thr, np.int32), t(mb, np.int32), W, H, **kw)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}, offs


def _check(imgs, thr, mb, out):
    """every slot against _reference; without descriptors (out["comp"] is None) kept_off, kept_idx, ncomp, nkept_comp and
    stats are checked, and that comp_off is still the exclusive scan of nkept_comp"""
    n = len(imgs)
    ko, co = out["kept_off"].astype(np.int64), out["comp_off"].astype(np.int64)
    fg = ncomp_total = nkept_total = 0
    for s in range(n):
        ncomp, comps, kept = _reference(imgs[s], thr[s], mb[s])
        fg += int((imgs[s] > thr[s]).sum())
        ncomp_total += ncomp
        nkept_total += len(comps)
        assert out["ncomp"][s] == ncomp, (s, out["ncomp"][s], ncomp)
        assert out["nkept_comp"][s] == len(comps)
        assert np.array_equal(out["kept_idx"][ko[s]:ko[s + 1]], kept), s
        assert co[s + 1] - co[s] == len(comps)
        if out["comp"] is None:
            continue
        got = [tuple(int(x) for x in r) for r in out["comp"][co[s]:co[s + 1]]]
        assert got == comps, (s, got[:5], comps[:5])
    if out["comp"] is None:
        assert co[0] == 0 and np.array_equal(np.diff(co), out["nkept_comp"])
    st = out["stats"]
    assert (st[1], st[2], st[3]) == (fg, ncomp_total, nkept_total)
    return st


def _assert_same_outputs(out, out2):
    """two launches wrote the same outputs: every array, but kept_idx and comp only up to their counts (the rest of those
    buffers is never written: torch.empty)"""
    for k in out:
        a, b = out[k], out2[k]
        if k == "kept_idx":
            a, b = a[:out["kept_off"][-1]], b[:out2["kept_off"][-1]]
        elif k == "comp":
            a, b = a[:out["comp_off"][-1]], b[:out2["comp_off"][-1]]
        assert np.array_equal(a, b), k


# ---- shapes -----------------------------------------------------------------------------------------------------------
# Every generator returns u8 [H, W] with FG on the shape and 0 elsewhere, for any H, W >= 1.  The component counts below
# are for 8-connectivity.

def _img(m):
    return np.where(m, FG, 0).astype(np.uint8)


def _yx(H, W):
    return np.mgrid[0:H, 0:W]


def serpentine(H, W):
    """every second row full; rows 2k and 2k+2 joined by one pixel of row 2k+1, at the right end for even k and at the
    left end for odd k: one snake of about W*H/2 pixels.  1 component (the rows alone would be ceil(H/2))."""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    for k in range((H - 1) // 2):
        m[2 * k + 1, W - 1 if k % 2 == 0 else 0] = True
    return _img(m)


def checkerboard(H, W):
    """(x + y) % 2 == 0: every link is diagonal.  1 component where H, W >= 2 (4-connectivity would give one per pixel);
    on a single row or column the pixels are isolated: ceil(max(H, W) / 2)."""
    y, x = _yx(H, W)
    return _img((x + y) % 2 == 0)


def diagonal(H, W):
    """np.eye: min(H, W) pixels, each linked to its NW neighbour only.  1 component."""
    return _img(np.eye(H, W, dtype=bool))


def antidiagonal(H, W):
    """np.fliplr(np.eye): each pixel linked to its NE neighbour only.  1 component."""
    return _img(np.fliplr(np.eye(H, W, dtype=bool)))


def diagonals(H, W):
    """stripes (x - y) % 3 == 0: NW-only links on a third of the frame.  Two stripes are 3 apart in x - y and a step to
    a neighbour changes x - y by at most 2, so they never touch: one component per c in [-(H-1), W-1] with c % 3 == 0."""
    y, x = _yx(H, W)
    return _img((x - y) % 3 == 0)


def antidiagonals(H, W):
    """stripes (x + y) % 3 == 0: NE-only links.  One component per c in [0, H+W-2] with c % 3 == 0."""
    y, x = _yx(H, W)
    return _img((x + y) % 3 == 0)


def hline(H, W, y):
    """row y full: W-only links.  1 component."""
    m = np.zeros((H, W), bool)
    m[y] = True
    return _img(m)


def vline(H, W, x):
    """column x full: N-only links.  1 component."""
    m = np.zeros((H, W), bool)
    m[:, x] = True
    return _img(m)


def hlines(H, W):
    """rows 0, 3, 6, ... full.  ceil(H / 3) components."""
    m = np.zeros((H, W), bool)
    m[0::3] = True
    return _img(m)


def vlines(H, W):
    """columns 0, 3, 6, ... full.  ceil(W / 3) components."""
    m = np.zeros((H, W), bool)
    m[:, 0::3] = True
    return _img(m)


def wrap_pair(H, W, y=0):
    """pixels (y, W-1) and (y+1, 0): adjacent raster indices, not neighbours.  2 components where W >= 3 and row y+1
    exists; with W <= 2 the two touch (1 component), with y+1 == H only the first pixel exists (1 component)."""
    m = np.zeros((H, W), bool)
    m[y, W - 1] = True
    if y + 1 < H:
        m[y + 1, 0] = True
    return _img(m)


def comb(H, W):
    """columns 0, 2, 4, ... full, joined only by the full bottom row: merges found last in raster order.  1 component
    (the teeth alone would be ceil(W / 2))."""
    m = np.zeros((H, W), bool)
    m[:, 0::2] = True
    m[H - 1] = True
    return _img(m)


def ring_boxes(H, W):
    """-> [(x0, y0, x1, y1)] of rings(): rectangle k is inset by 2k, as long as it is at least 3 x 3"""
    out, k = [], 0
    while min(H, W) - 1 - 4 * k >= 2:
        out.append((2 * k, 2 * k, W - 1 - 2 * k, H - 1 - 2 * k))
        k += 1
    return out


def rings(H, W):
    """concentric one-pixel rectangle outlines, 2 apart (one background pixel between two rings), each at least 3 x 3:
    nested, none merged.  One component per ring: (min(H, W) - 3) // 4 + 1, none where min(H, W) < 3."""
    m = np.zeros((H, W), bool)
    for x0, y0, x1, y1 in ring_boxes(H, W):
        m[y0, x0:x1 + 1] = m[y1, x0:x1 + 1] = True
        m[y0:y1 + 1, x0] = m[y0:y1 + 1, x1] = True
    return _img(m)


def corners(H, W):
    """the four corner pixels.  4 components where H, W >= 3; corners of a side of length <= 2 coincide or touch, so in
    general (1 if H <= 2 else 2) * (1 if W <= 2 else 2)."""
    m = np.zeros((H, W), bool)
    m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = True
    return _img(m)


def lattice_capacity(H, W):
    return ((H + 1) // 2) * ((W + 1) // 2)


def lattice(H, W, n, seed=0, avoid=None):
    """exactly n isolated pixels drawn (seeded) from the even-row, even-column lattice; with `avoid` (an image) none within
    2 pixels of its foreground, so the union with it has n more components.  n components, values 1 .. 255."""
    free = np.zeros((H, W), bool)
    free[0::2, 0::2] = True
    if avoid is not None:
        from scipy import ndimage

        free &= ~ndimage.binary_dilation(avoid > 0, structure=np.ones((5, 5)))
    pos = np.flatnonzero(free.ravel())
    if n > len(pos):
        raise ValueError(f"lattice: {n} pixels asked, {len(pos)} places")
    rs = np.random.RandomState(seed)
    pick = rs.choice(pos, n, replace=False)
    v = np.zeros(H * W, np.uint8)
    v[pick] = rs.randint(1, 256, n)
    return v.reshape(H, W)


def compact(H, W, n, x=0, y=0):
    """one compact blob of exactly n pixels with its corner at (x, y): a filled rectangle plus a partial row below it.
    1 component (n >= 1)."""
    w = min(W - x, max(int(np.ceil(np.sqrt(n))), -(-n // (H - y))))
    rows, rem = divmod(n, w)
    if rows + (rem > 0) > H - y:
        raise ValueError("compact: does not fit")
    m = np.zeros((H, W), bool)
    m[y:y + rows, x:x + w] = True
    m[y + rows:y + rows + 1, x:x + rem] = True
    return _img(m)


def _count_mod3(lo, hi):
    return sum(1 for c in range(lo, hi + 1) if c % 3 == 0)


# name -> (generator(H, W), components(H, W), nested): every row of the table but lattice (n is its parameter)
SHAPES = {
    "serpentine": (serpentine, lambda H, W: 1, False),
    "checkerboard": (checkerboard, lambda H, W: 1 if min(H, W) >= 2 else (max(H, W) + 1) // 2, False),
    "diagonal": (diagonal, lambda H, W: 1, False),
    "antidiagonal": (antidiagonal, lambda H, W: 1, False),
    "diagonals": (diagonals, lambda H, W: _count_mod3(-(H - 1), W - 1), False),
    "antidiagonals": (antidiagonals, lambda H, W: _count_mod3(0, H + W - 2), False),
    "hline_top": (lambda H, W: hline(H, W, 0), lambda H, W: 1, False),
    "hline_bottom": (lambda H, W: hline(H, W, H - 1), lambda H, W: 1, False),
    "vline_left": (lambda H, W: vline(H, W, 0), lambda H, W: 1, False),
    "vline_right": (lambda H, W: vline(H, W, W - 1), lambda H, W: 1, False),
    "hlines": (hlines, lambda H, W: (H + 2) // 3, False),
    "vlines": (vlines, lambda H, W: (W + 2) // 3, False),
    "wrap_pair": (wrap_pair, lambda H, W: 2 if W >= 3 and H >= 2 else 1, False),
    "comb": (comb, lambda H, W: 1, False),
    "rings": (rings, lambda H, W: (min(H, W) - 3) // 4 + 1 if min(H, W) >= 3 else 0, True),
    "corners": (corners, lambda H, W: (1 if H <= 2 else 2) * (1 if W <= 2 else 2), False),
}
