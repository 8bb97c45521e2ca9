"""The K4b scenes and their reference, pinned on the CPU: the GPU tests (test_gpu_blobs.py, test_gpu_blobs_limits.py)
compare the kernels with blobscenes._reference on blobscenes' shapes, so the component counts the module states, the
reference itself (against a plain flood fill written here) and the tie to what the localizer's contour finder sees are
checked without a GPU."""
import numpy as np
import pytest

import blobscenes as bs

SMALL = [(24, 40), (37, 322)]
SIZES = SMALL + [(1, 17), (17, 1), (2, 2)]


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("name", list(bs.SHAPES))
def test_shape_has_the_stated_component_count(name, H, W):
    gen, count, _ = bs.SHAPES[name]
    v = gen(H, W)
    assert v.shape == (H, W) and v.dtype == np.uint8
    ncomp, comps, kept = bs._reference(v, 0, -1)
    assert ncomp == count(H, W) == len(comps)
    assert np.array_equal(kept, np.flatnonzero(v.ravel()))  # min_box_area = -1: the kept pixels are the foreground
    assert sum(c[5] for c in comps) == len(kept)


def test_counts_at_three_sizes():
    """the stated counts as plain numbers at 24x40, 37x322 and 1050x1680 (scipy at the two small sizes)"""
    want = {"serpentine": (1, 1, 1), "checkerboard": (1, 1, 1), "wrap_pair": (2, 2, 2), "comb": (1, 1, 1),
            "diagonal": (1, 1, 1), "antidiagonal": (1, 1, 1), "rings": (6, 9, 262), "diagonals": (21, 120, 909),
            "antidiagonals": (21, 120, 910), "hlines": (8, 13, 350), "vlines": (14, 108, 560)}
    for name, exp in want.items():
        gen, count, _ = bs.SHAPES[name]
        for (H, W), e in zip(SMALL + [(1050, 1680)], exp):
            assert count(H, W) == e, (name, H, W)
            if H < 1000:
                assert bs._reference(gen(H, W), 0, -1)[0] == e, (name, H, W)


@pytest.mark.parametrize("name", ["serpentine", "checkerboard", "antidiagonals", "rings", "comb"])
def test_full_size_shapes(name):
    H, W = 1050, 1680
    gen, count, _ = bs.SHAPES[name]
    v = gen(H, W)
    assert (v > 0).sum() > bs.LDS_N  # a dense-plane scene
    ncomp, comps, kept = bs._reference(v, 0, 10)
    assert ncomp == count(H, W)
    if name == "rings":
        assert [c[1:5] for c in comps] == bs.ring_boxes(H, W)


def test_rings_are_their_rectangles():
    for H, W in SMALL:
        boxes = bs.ring_boxes(H, W)
        ncomp, comps, _ = bs._reference(bs.rings(H, W), 0, -1)
        assert ncomp == len(boxes) > 1
        for (first, x0, y0, x1, y1, npix), b in zip(comps, boxes):
            assert (x0, y0, x1, y1) == b and first == y0 * W + x0
            assert npix == 2 * (x1 - x0 + 1) + 2 * (y1 - y0 + 1) - 4


def _flood(m):
    """8-connected components of a bool image by flood fill: -> [(first, x0, y0, x1, y1, npix)] in raster order of the
    first pixel, and a label image (component number + 1, 0 = background)"""
    H, W = m.shape
    lab = np.zeros((H, W), np.int64)
    comps = []
    for y in range(H):
        for x in range(W):
            if not m[y, x] or lab[y, x]:
                continue
            k = len(comps) + 1
            lab[y, x] = k
            stack, x0, y0, x1, y1, npix = [(y, x)], x, y, x, y, 0
            while stack:
                cy, cx = stack.pop()
                npix += 1
                x0, x1, y0, y1 = min(x0, cx), max(x1, cx), min(y0, cy), max(y1, cy)
                for ny in range(max(cy - 1, 0), min(cy + 2, H)):
                    for nx in range(max(cx - 1, 0), min(cx + 2, W)):
                        if m[ny, nx] and not lab[ny, nx]:
                            lab[ny, nx] = k
                            stack.append((ny, nx))
            comps.append((y * W + x, x0, y0, x1, y1, npix))
    return comps, lab


def _flood_cases(H, W):
    rs = np.random.RandomState(H * W)
    for name, (gen, _, _) in bs.SHAPES.items():
        yield name, gen(H, W), 0
    yield "lattice", bs.lattice(H, W, 100, seed=3), 0
    yield "lattice+diagonal", np.maximum(bs.diagonal(H, W), bs.lattice(H, W, 60, seed=4, avoid=bs.diagonal(H, W))), 0
    yield "compact", bs.compact(H, W, 333, x=3, y=2), 0
    yield "scatter", bs._slot_image(rs, W, H, "small"), 40
    yield "dense", bs._slot_image(rs, W, H, "large"), 0


@pytest.mark.parametrize("H,W", SMALL)
def test_reference_equals_flood_fill(H, W):
    for name, v, thr in _flood_cases(H, W):
        comps, lab = _flood(v > thr)
        for mb in (-1, 0, 10):
            ncomp, rcomps, rkept = bs._reference(v, thr, mb)
            keep = [mb < 0 or (c[3] - c[1] + 1) * (c[4] - c[2] + 1) > mb for c in comps]
            assert ncomp == len(comps), (name, mb)
            assert rcomps == [c for c, k in zip(comps, keep) if k], (name, mb)
            kept = np.flatnonzero(np.concatenate([[False], keep])[lab].ravel())
            assert np.array_equal(rkept, kept), (name, mb)


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2047, 2048, 2049])
def test_lattice_has_exactly_n_isolated_pixels(n):
    H, W = 1050, 1680
    v = bs.lattice(H, W, n, seed=n)
    assert (v > 0).sum() == n
    ncomp, comps, kept = bs._reference(v, 0, 0)
    assert ncomp == n == len(comps) == len(kept)
    assert all(c[5] == 1 for c in comps)
    assert bs._reference(v, 0, 10)[1] == []  # boxes of area 1: a minimum of 10 keeps nothing


def test_lattice_keeps_away_from_the_shape_it_shares_a_slot_with():
    H, W = 37, 322
    for name in ("wrap_pair", "corners", "hline_bottom", "vline_right", "antidiagonal"):
        gen, count, _ = bs.SHAPES[name]
        shape = gen(H, W)
        lat = bs.lattice(H, W, 2049, seed=1, avoid=shape)
        assert not ((shape > 0) & (lat > 0)).any() and (lat > 0).sum() == 2049
        assert bs._reference(np.maximum(shape, lat), 0, -1)[0] == count(H, W) + 2049, name
    with pytest.raises(ValueError):
        bs.lattice(H, W, bs.lattice_capacity(H, W) + 1)


def test_compact_has_exactly_n_pixels_in_one_component():
    for H, W in [(37, 322), (1050, 1680)]:
        for n in (1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 2050):
            v = bs.compact(H, W, n, x=5, y=0)
            ncomp, comps, _ = bs._reference(v, 0, -1)
            assert (v > 0).sum() == n and ncomp == 1 and comps[0][5] == n, (H, W, n)


@pytest.mark.parametrize("H,W", SIZES)
def test_contour_finder_sees_one_external_contour_per_component(oracle, H, W):
    """without nesting, RETR_EXTERNAL reports one contour per 8-connected component: what K4b keeps or drops is what the
    localizer would have traced"""
    for name, (gen, count, nested) in bs.SHAPES.items():
        v = gen(H, W)
        n = len(oracle.find_contours((v > 0).astype(np.uint8) * 255)) if v.any() else 0
        if nested:
            assert n == min(count(H, W), 1), name  # only the outermost ring is external
        else:
            assert n == count(H, W) == bs._reference(v, 0, -1)[0], name
    lat = bs.lattice(H, W, min(50, bs.lattice_capacity(H, W)), seed=9)
    assert len(oracle.find_contours((lat > 0).astype(np.uint8) * 255)) == (lat > 0).sum()
