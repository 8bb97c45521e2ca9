"""CPU-side checks of the blob labelling (K4b, abub_blobs.hip) and its pipeline knob: the entries are declared, exported
and bound, the knob setter validates without a device, and the argument that makes the box filter exact holds on the
host's own contour finder."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from autobub3hs_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("abub_binarize_thr_dev", "abub_label_blobs_dev", "abub_label_blobs_scratch_bytes")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def test_new_entries_declared_exported_and_bound():
    from autobub3hs_amd import hip

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "abub_hip.h")).read(), flags=re.S)
    L = C.CDLL(_lib.build())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert callable(hip.binarize_thr) and callable(hip.label_blobs)
    # scratch sizing needs no device; impossible shapes give 0
    lib = _lib.lib()
    assert lib.abub_label_blobs_scratch_bytes(10, 1280, 1024, 1 << 20, 0) > 0
    assert lib.abub_label_blobs_scratch_bytes(10, 1280, 1024, 1 << 20, 1) > lib.abub_label_blobs_scratch_bytes(10, 1280, 1024,
                                                                                                               1 << 20, 0)
    assert lib.abub_label_blobs_scratch_bytes(0, 1280, 1024, 16, 0) == 0
    assert lib.abub_label_blobs_scratch_bytes(4, 0, 1024, 16, 0) == 0


def test_pipeline_option_setter_refuses_bad_names_and_values():
    L = host.lib()
    L.abh_pipe_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.abh_pipe_error.restype = C.c_char_p
    assert L.abh_pipe_set_option(None, b"no_such_option", 1) == -1
    assert b"unknown option" in L.abh_pipe_error()
    assert L.abh_pipe_set_option(None, None, 1) == -1
    for v in (-1, 2, 7):
        assert L.abh_pipe_set_option(None, b"blobs", v) == -1
        assert b"0 or 1" in L.abh_pipe_error()
    assert L.abh_pipe_set_option(None, b"blobs", 1) == -1  # valid name and value, but no pipeline
    assert b"no pipeline" in L.abh_pipe_error()


def test_label_blobs_refuses_bad_arguments_before_the_device():
    lib = _lib.lib()
    z = C.c_void_p(0)
    args = [z, z, z, 16, 4, 64, 64, z, z, z, z, 16, z, z, z, None, 0, z, z, 0, None]
    assert lib.abub_label_blobs_dev(*args) == -1
    assert b"bad arguments" in lib.abub_last_error()
    assert lib.abub_binarize_thr_dev(None, None, 4, 64, 64, None, None) == -1


# ---- the filtering argument, on the host's contour finder ------------------------------------------------------------

def _box_area(xy):
    return int((xy[:, 0].max() - xy[:, 0].min() + 1) * (xy[:, 1].max() - xy[:, 1].min() + 1))


def _masks(rs):
    """random masks of the kinds that could break the argument"""
    out = []
    for _ in range(60):  # sparse noise
        H, W = rs.randint(1, 40), rs.randint(1, 40)
        out.append(rs.rand(H, W) < rs.choice([0.05, 0.2, 0.4, 0.6]))
    for _ in range(60):  # rings with components inside their holes, touching the edges and corners
        H, W = rs.randint(6, 40), rs.randint(6, 40)
        m = rs.rand(H, W) < 0.08
        for _ in range(rs.randint(1, 4)):
            h, w = rs.randint(3, 12), rs.randint(3, 12)
            y, x = rs.randint(-2, H - 1), rs.randint(-2, W - 1)
            y0, y1, x0, x1 = max(y, 0), min(y + h, H), max(x, 0), min(x + w, W)
            if y1 - y0 < 1 or x1 - x0 < 1:
                continue
            m[y0:y1, x0:x1] = True
            m[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = False
            iy, ix = (y0 + y1) // 2, (x0 + x1) // 2
            m[iy, ix] = True  # a dot (or more) inside the hole
            if rs.rand() < 0.5 and iy + 1 < y1 - 1:
                m[iy + 1, ix] = True
        out.append(m)
    for _ in range(40):  # blobs of every size near the 10-pixel box limit
        H, W = rs.randint(5, 30), rs.randint(5, 30)
        m = np.zeros((H, W), bool)
        for _ in range(rs.randint(1, 8)):
            h, w = rs.randint(1, 6), rs.randint(1, 6)
            y, x = rs.randint(0, H), rs.randint(0, W)
            m[y:y + h, x:x + w] = rs.rand(min(h, H - y), min(w, W - x)) < 0.8
        out.append(m)
    for _ in range(40):  # one row, one column
        n = rs.randint(1, 80)
        m = rs.rand(n) < rs.choice([0.3, 0.7])
        out.append(m[None, :] if rs.rand() < 0.5 else m[:, None])
    out.append(np.ones((5, 5), bool))
    ring = np.ones((5, 5), bool)
    ring[1:4, 1:4] = False
    ring[2, 2] = True
    out.append(ring)  # the smallest enclosing ring: box area 25
    return out


def test_box_filter_keeps_every_contour_tracking_uses(oracle):
    from scipy import ndimage

    rs = np.random.RandomState(11)
    masks = _masks(rs)
    assert len(masks) >= 200
    for m in masks:
        H, W = m.shape
        lab, n = ndimage.label(m, structure=np.ones((3, 3)))
        keep = np.zeros(n + 1, bool)
        for k, sl in enumerate(ndimage.find_objects(lab), start=1):
            keep[k] = (sl[0].stop - sl[0].start) * (sl[1].stop - sl[1].start) > 10
        kept = np.flatnonzero(keep[lab].ravel() & m.ravel()).astype(np.uint32)
        got = [c for c in (host.contours_from_indices(kept, W, H) if len(kept) else []) if _box_area(c) > 10]
        ref = [xy for xy, _ in oracle.find_contours(m.astype(np.uint8) * 255) if _box_area(xy) > 10]
        assert len(got) == len(ref), (m.astype(int), len(got), len(ref))
        for a, b in zip(got, ref):
            assert np.array_equal(a, b)
