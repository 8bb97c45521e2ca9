"""Pins the CPU oracle at the edges the GPU edge tests (test_gpu_edges.py) compare against: FindTriggerFrame at every
stack length and trigger position of those tests against the independent restatement in pyref, and Otsu / binarize on
degenerate histograms against the numpy restatement of test_oracle_primitives.  A GPU failure at these edges then points
at the product, not at the oracle."""
import numpy as np
import pytest

import edgescenes
import pyref
from autobub3hs_amd import synth
from test_oracle_primitives import np_otsu


@pytest.mark.parametrize("F", edgescenes.STACK_LENGTHS)
@pytest.mark.parametrize("tss", [4, 16])  # one-frame offset and threshold 5 / two-frame offset and threshold 3.5
def test_find_trigger_at_stack_length_edges(oracle, F, tss):
    W, H = 128, 64
    mu, sg = oracle.welford(synth.training_pairs(W, H, tss // 2, 0, 30))
    frames, onsets = edgescenes.trigger_stacks(W, H, F, seed=F)
    found = []
    for e, t in enumerate(onsets):
        a = oracle.Analyzer(frames[e], mu, sg, tss)
        st = a.find_trigger(1)
        a.close()
        status, trig, ok, sobj = pyref.find_trigger(list(frames[e]), sg, tss)
        assert (st["status"], st["ok"]) == (status, ok), (F, tss, t, st, status)
        if F < 5:
            assert status == -9  # AnalyzerUnit.cpp:122-126
            continue
        assert st["loc_thres"] == sobj.loc_thres, (F, tss, t)
        if status == 0:
            assert st["trig"] == trig == t, (F, tss, t, st["trig"], trig)
            found.append(t)
        else:
            assert status == -3
    if F >= 5:
        # the look-ahead needs two frames behind the trigger: a bubble that starts at F - 2 or F - 1 is never confirmed,
        # one at F - 3 (and at every other planned position) is
        assert found == [t for t in onsets if t is not None and t <= F - 3], (F, tss, found)


def _degenerate_images(H=24, W=40):
    """name -> image whose histogram is degenerate: all pixels in one bin (0, 1, 3, 4, 128, 255), only the values 0 and 255
    (balanced, one 255 pixel, one 0 pixel), only bin 255."""
    out = {}
    for v in (0, 1, 3, 4, 128, 255):
        out[f"one_bin_{v}"] = np.full((H, W), v, np.uint8)
    img = np.zeros((H, W), np.uint8)
    img[:, W // 2:] = 255
    out["halves_0_255"] = img
    img = np.zeros((H, W), np.uint8)
    img[H - 1, W - 1] = 255
    out["one_255_in_zeros"] = img
    img = np.full((H, W), 255, np.uint8)
    img[0, 0] = 0
    out["one_0_in_255"] = img
    return out


@pytest.mark.parametrize("name,img", list(_degenerate_images().items()))
def test_otsu_and_binarize_degenerate_histograms(oracle, name, img):
    h = np.bincount(img.ravel(), minlength=256).astype(np.uint32)
    assert oracle.otsu(h) == np_otsu(h), name
    if (h > 0).sum() == 1:
        assert oracle.otsu(h) == 0  # one bin: no split is ever admissible (q1 or q2 below FLT_EPSILON)
    for tozero in (0, 3, 128, 254, 255):
        t = np.where(img > tozero, img, 0)
        ht = np.bincount(t.ravel(), minlength=256)
        m, T = oracle.binarize(img, tozero)
        assert T == np_otsu(ht), (name, tozero)
        assert np.array_equal(m, np.where(t > T, 255, 0).astype(np.uint8)), (name, tozero)
