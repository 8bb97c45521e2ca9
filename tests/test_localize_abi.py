"""CPU-side checks of the device localizer (K7, abub_localize.hip): its entries declared, exported and bound, limits that
answer without a device, bad arguments and bad knob values refused before the device; and the reference side the GPU tests
stand on (locscenes.py): describe() against the host's probe, the contour-driven reference localizer against the oracle's
event results on the oracle's polygons, and the hand-made stacks against what they promise."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import locscenes as ls
from autobub3hs_amd import _lib, host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"abub_describe_contours_dev": "L3Localizer.cpp:401-418 and :808-823",
       "abub_localize_stacks_dev": "L3Localizer.cpp:215-460, 764-869, 971-1012",
       "abub_localize_scratch_bytes": "L3Localizer.cpp:215-460, 764-869, 971-1012",
       "abub_localize_limits": "L3Localizer.cpp:215-460, 764-869, 971-1012"}


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def limits():
    mc, mb = C.c_int(-1), C.c_int(-1)
    assert _lib.lib().abub_localize_limits(C.byref(mc), C.byref(mb)) == 0
    return mc.value, mb.value


# ---- (a) the C surface ---------------------------------------------------------------------------------------------
def test_new_entries_declared_exported_and_bound():
    from autobub3hs_amd import hip

    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = C.CDLL(_lib.build())
    for name, cite in NEW.items():
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
        before = hdr[:hdr.index(name + "(")]
        assert cite in re.sub(r"\n \*", "", before[before.rindex("/*"):]), name
    for rec, size in ((_lib.ContourDesc, 80), (_lib.LocStack, 64), (_lib.LocMask, 32)):
        assert C.sizeof(rec) == size
    assert ls.DESC.itemsize == 80 and hip.desc_dtype() == ls.DESC
    assert [n for n, _ in _lib.ContourDesc._fields_] == list(ls.DESC.names)
    for word in ("abub_contour_desc", "abub_loc_stack", "abub_loc_mask", "abub_loc_result", "ABUB_LOC_BELLOWS"):
        assert word in txt, word
    for k, v in (("DONE", 0), ("LIMIT", 1), ("SLOT", 2), ("BAD_FRAME", 3), ("BELLOWS", 4), ("INCOMPLETE", 5)):
        assert re.search(r"#define ABUB_LOC_%s %d\b" % (k, v), txt) and getattr(ls, k) == v and getattr(hip, "LOC_" + k) == v
    assert re.search(r"#define ABUB_LOC_MAXTRACK %d\b" % ls.MAXTRACK, txt) and _lib.LOC_MAXTRACK == ls.MAXTRACK
    assert callable(hip.describe_contours) and callable(hip.localize_stacks) and callable(hip.localize_limits)
    assert "abh_pipe_localize_stats" in host.SIGNATURES and callable(host.Pipeline.localize_stats)


def test_limits_and_sizes_need_no_device():
    lib = _lib.lib()
    mc, mb = limits()
    assert mc >= 64 and 1 <= mb <= 64
    assert lib.abub_localize_limits(None, None) == 0
    assert lib.abub_localize_scratch_bytes(4, 3) >= 4 * 64 + 3 * 32
    assert lib.abub_localize_scratch_bytes(0, 2) == 0 and lib.abub_localize_scratch_bytes(-1, 2) == 0
    assert lib.abub_localize_scratch_bytes(3, 0) == 0


def test_describe_refuses_bad_arguments_before_the_device():
    lib = _lib.lib()
    one = C.c_void_p(256)  # never dereferenced: every call below is refused while the arguments are checked
    # (status, cont_off, cont_npts, cont_cap, pt_off, pts, pts_cap, nslots, desc, desc_cap, stream)
    good = [one, one, one, 16, one, one, 64, 4, one, 16, None]
    for pos, bad in ((0, None), (1, None), (2, None), (4, None), (5, None), (8, None), (3, 0), (6, 0), (9, 0), (7, -1),
                     (3, 1 << 31), (6, 1 << 31), (9, 1 << 31)):
        args = list(good)
        args[pos] = bad
        assert lib.abub_describe_contours_dev(*args) == -1, pos
        assert b"abub_describe_contours_dev: bad arguments" in lib.abub_last_error(), pos
    args = list(good)
    args[7] = 0  # nothing to do
    assert lib.abub_describe_contours_dev(*args) == 0


def test_localize_refuses_bad_arguments_before_the_device():
    lib = _lib.lib()
    one = C.c_void_p(256)
    st = (_lib.LocStack * 2)()
    mk = (_lib.LocMask * 2)()
    for k in range(2):
        st[k].cam, st[k].genesis, st[k].ntrack, st[k].bad = k, 3 * k, 2, 0
        st[k].track[0], st[k].track[1] = 3 * k + 1, 3 * k + 2
    mk[1].fid, mk[1].fw, mk[1].fh = 256, 64, 48
    S, M = C.addressof(st), C.addressof(mk)
    # (stacks, nstacks, masks, ncams, slot_status, cont_off, nslots, desc, ndesc, scratch, scratch_bytes, out, rects,
    #  rect_cap, tracks, track_cap, totals, stream)
    good = [S, 2, M, 2, one, one, 6, one, 10, one, 1 << 16, one, one, 8, one, 8, one, None]
    for pos, bad in ((0, None), (2, None), (4, None), (5, None), (7, None), (9, None), (11, None), (12, None), (14, None),
                     (16, None), (1, -1), (3, 0), (3, -1), (6, 0), (6, -2), (13, 0), (15, 0)):
        args = list(good)
        args[pos] = bad
        assert lib.abub_localize_stacks_dev(*args) == -1, pos
        assert b"abub_localize_stacks_dev: bad arguments" in lib.abub_last_error(), pos
    args = list(good)
    args[10] = 8
    assert lib.abub_localize_stacks_dev(*args) == -1 and b"scratch" in lib.abub_last_error()
    args = list(good)
    args[9] = C.c_void_p(264)
    assert lib.abub_localize_stacks_dev(*args) == -1 and b"scratch" in lib.abub_last_error()

    def refused(word):
        assert lib.abub_localize_stacks_dev(*good) == -1 and word in lib.abub_last_error(), lib.abub_last_error()

    st[1].ntrack = ls.MAXTRACK + 1
    refused(b"more tracking slots")
    st[1].ntrack = -1
    refused(b"more tracking slots")
    st[1].ntrack = 2
    for field, bad in (("cam", 2), ("cam", -1), ("genesis", 6), ("genesis", -1)):
        keep = getattr(st[1], field)
        setattr(st[1], field, bad)
        refused(b"bad stack descriptor")
        setattr(st[1], field, keep)
    st[1].track[1] = 6
    refused(b"bad stack descriptor")
    st[1].track[1] = 5
    mk[1].fw = 0
    refused(b"bad mask descriptor")
    mk[1].fw = 64
    mk[0].bel, mk[0].bw, mk[0].bh = 256, 64, -1
    refused(b"bad mask descriptor")
    args = list(good)
    args[1] = 0  # nothing to do
    assert lib.abub_localize_stacks_dev(*args) == 0


def test_pipeline_option_localize_is_known_and_validated():
    L = host.lib()
    L.abh_pipe_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.abh_pipe_error.restype = C.c_char_p
    assert L.abh_pipe_set_option(None, b"localize", 1) == -1  # valid name and value, but no pipeline
    assert b"no pipeline" in L.abh_pipe_error()
    assert b"unknown option" not in L.abh_pipe_error()
    for v in (-1, 2):
        assert L.abh_pipe_set_option(None, b"localize", v) == -1
        assert b"takes 0 or 1" in L.abh_pipe_error()


# ---- (b) the reference side ----------------------------------------------------------------------------------------
def test_describe_restates_the_host_probe():
    rs = np.random.RandomState(7)
    polys = ls.random_polygons(rs, 400, nmax=300)
    nan = zero = 0
    for p in polys:
        a, b = ls.describe(p), ls.host_record(p)
        assert ls.same_bits(a, b), (p[:8], a, b)
        nan += bool(np.isnan(a["cx"]))
        zero += a["m00"] == 0
        if a["m00"] == 0:  # the genesis fallback: the vertex mean
            assert a["gx"] == np.float32(p[:, 0].sum() / len(p)) and not np.isnan(a["gy"])
    assert nan >= 50 and zero >= 50 and zero < 300


def oracle_slots(oracle, fr, mu, sg, tss, t, loc_thres):
    """the polygons of the localizer's images of trigger t as the oracle's findContours returns them: genesis first"""
    F = len(fr)
    pre = max(t - (1 if tss < 6 else 2), 0)
    imgs = [(oracle.process_frame(fr[t], fr[pre], sg), loc_thres)]
    last = ls.MAXTRACK if t < 29 else 39 - t
    for k in range(1, last + 1):
        if t + k >= F:
            break
        imgs.append((oracle.posttrig_frame(fr[t + k], mu, sg), 3))
    slots = []
    for img, tz in imgs:
        mask, _ = oracle.binarize(img, tz)
        slots.append([ls.describe(xy) for xy, _ in oracle.find_contours(mask)])
    return slots


RENDERED = [(W, H, masked, e) for (W, H) in ((96, 160), (200, 120)) for masked in (0, 1) for e in range(10)]


@pytest.fixture(scope="module")
def models(oracle):
    out = {}
    for (W, H) in ((96, 160), (200, 120)):
        for cam in (0, 1):
            tr = synth.training_pairs(W, H, 5, cam, 41)
            out[W, H, cam] = oracle.welford(tr) + (len(tr),)
    return out


@pytest.mark.parametrize("W,H,masked,e", RENDERED)
def test_reference_localizer_follows_the_oracle(oracle, models, W, H, masked, e):
    """ref_localize on the oracle's polygons against the oracle's localize() of the same trigger: the same bubbles with
    the same descriptors in the same order (boxes exactly, the double columns to 1e-4 like every event comparison)"""
    cam, F = e % 2, 41
    mu, sg, tss = models[W, H, cam]
    fid, bel = synth.camera_masks(W, H, cam) if masked else (None, None)
    spec = synth.random_spec(W, H, F, 4100 + e, cam, p_second=0.5, p_flicker=0.2, margin=min(25, W // 4))
    fr = synth.render_event(W, H, spec, 4100 + e, cam)
    a = oracle.Analyzer(fr, mu, sg, tss, fid_mask=fid, bel_mask=bel)
    st = a.find_trigger(1)
    if not st["ok"]:
        a.close()
        return  # no trigger in this stack (test_rendered_set_reaches_bubbles_and_tracks counts the ones that have one)
    bubbles = a.localize()
    a.close()
    slots = oracle_slots(oracle, fr, mu, sg, tss, st["trig"], st["loc_thres"])
    status, off, desc = ls.pack(slots)
    mc, mb = limits()
    stack = {"cam": 0, "genesis": 0, "track": list(range(1, len(slots))), "bad": 0}
    r = ls.ref_localize(stack, [(fid, bel)], status, off, desc, len(desc), mc, mb)
    if r["status"] == ls.BELLOWS:  # without a template the oracle goes on with every contour: the host's branch
        return
    assert r["status"] == ls.DONE  # rendered stacks stay inside the limits
    assert len(r["bubbles"]) == len(bubbles)
    for mine, ref in zip(r["bubbles"], bubbles):
        assert len(mine) == len(ref["desc"])
        for j, (k, d) in enumerate(zip(mine, ref["desc"])):
            assert tuple(int(desc[k][c]) for c in "xywh") == tuple(d[c] for c in "xywh")
            for c in ("area", "radius", "m00", "m10", "m01", "cx", "cy"):
                v = float(desc[k]["gx" if c == "cx" and j == 0 else "gy" if c == "cy" and j == 0 else c])
                if np.isnan(d[c]):
                    assert np.isnan(v)
                else:
                    assert abs(v - d[c]) <= 1e-4 * max(1.0, abs(d[c])), (c, v, d[c])


def test_rendered_set_reaches_bubbles_and_tracks(oracle, models):
    """the rendered set is no empty promise: most stacks trigger, bubbles are tracked over several frames, and the masks
    drop something"""
    trig = tracked = 0
    for (W, H, masked, e) in RENDERED[::3]:
        cam = e % 2
        mu, sg, tss = models[W, H, cam]
        spec = synth.random_spec(W, H, 41, 4100 + e, cam, p_second=0.5, p_flicker=0.2, margin=min(25, W // 4))
        a = oracle.Analyzer(synth.render_event(W, H, spec, 4100 + e, cam), mu, sg, tss)
        if a.find_trigger(1)["ok"]:
            trig += 1
            tracked += any(len(b["desc"]) >= 3 for b in a.localize())
        a.close()
    assert trig >= 10 and tracked >= 8, (trig, tracked)


def test_hand_made_stacks_hold_what_they_promise():
    mc, mb = limits()
    slots, stacks, masks, expect = ls.hand_made(mc, mb)
    status, off, desc = ls.pack(slots)
    seen = set()
    for i, (s, e) in enumerate(zip(stacks, expect)):
        r = ls.ref_localize(s, masks, status, off, desc, len(desc), mc, mb)
        seen.add(r["status"])
        assert r["status"] == e[0], (i, r, e)
        assert len(r["rects"]) == e[1], (i, r, e)
        assert [len(b) for b in r["bubbles"]] == e[2], (i, r, e)
    assert seen == {ls.DONE, ls.LIMIT, ls.SLOT, ls.BAD_FRAME, ls.BELLOWS}
    # records beyond ndesc: the lists overflowed, the stack is incomplete
    r = ls.ref_localize(stacks[-1], masks, status, off, desc, int(off[stacks[-1]["genesis"] + 1]) - 1, mc, mb)
    assert r["status"] == ls.INCOMPLETE


@pytest.mark.parametrize("regime", ["default", "post_trigger_dense", "noisy"])
def test_pipeline_regime_seeds_stay_inside_the_limits(oracle, regime):
    """the stacks test_gpu_localize_pipeline.py runs in each regime, localised round by round on the CPU (the retry of a
    trigger without an accepted bubble included): the reference localizer finishes every one of them -- no slot over the
    contour limit, no stack over the bubble limit -- which is why that test may demand an empty host route"""
    mc, mb = limits()
    slab, models, tss = ls.regime_run(oracle, regime)
    most = rounds = 0
    for e in range(slab.shape[0]):
        for c in range(slab.shape[1]):
            mu, sg = models[c]
            a = oracle.Analyzer(slab[e, c], mu, sg, tss[c])
            start = 1
            while True:
                st = a.find_trigger(start)
                if not st["ok"]:
                    break
                slots = oracle_slots(oracle, slab[e, c], mu, sg, tss[c], st["trig"], st["loc_thres"])
                status, off, desc = ls.pack(slots)
                stack = {"cam": 0, "genesis": 0, "track": list(range(1, len(slots))), "bad": 0}
                r = ls.ref_localize(stack, [(None, None)], status, off, desc, len(desc), mc, mb)
                assert r["status"] == ls.DONE, (regime, e, c, st, [len(s) for s in slots])
                most = max([most] + [len(s) for s in slots])
                rounds += 1
                if r["bubbles"]:
                    break
                start = st["trig"] + 1
            a.close()
    assert rounds >= 8 and most <= mc, (rounds, most)
    print(regime, "localisations", rounds, "most contours in a slot", most)
