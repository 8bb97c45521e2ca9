"""CPU-side checks of the device trigger search (K6, abub_trigger.hip): the histogram-driven reference model against the
oracle's FindTriggerFrame, the entries declared, exported and bound, limits that answer without a device, bad arguments
and bad knob values refused before the device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import pyref
import trigscenes as ts
from autobub3hs_amd import _lib, host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("abub_trigger_search_dev", "abub_trigger_search_desc_bytes", "abub_trigger_search_limits",
       "abub_trigger_clear_pending_dev")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def _stack_hists(oracle, fr, sg, tss):
    off = 1 if tss < 6 else 2
    h = np.zeros((len(fr), 256), np.uint32)
    for i in range(1, len(fr)):
        h[i] = oracle.hist256(oracle.process_frame(fr[i], fr[max(i - off, 0)], sg))
    return h


RENDERED = [(F, tss, ev) for F in (12, 41) for tss in (2, 10) for ev in (1, 2, 3)]


@pytest.mark.parametrize("F,tss,event", RENDERED)
def test_reference_model_follows_the_oracle(oracle, F, tss, event):
    """ref_search on the oracle's histograms against oracle.Analyzer.find_trigger on the frames: first search, and every
    retry from trig + 1 until the stack ends; with pyref.Sig and with the host's significance."""
    W, H = 32, 16
    t0 = 4 + event if F == 12 else 11 + 6 * event
    spec = (synth.EventSpec(F, t0, [(16, 8, -40)]), synth.EventSpec(F, t0, [(12, 7, 40)], flicker=t0 - 3, flicker_adu=12),
            synth.EventSpec(F, None, [], flicker=F // 2, flicker_adu=12))[event - 1]
    fr = synth.render_event(W, H, spec, event, 0)
    sg = np.zeros((H, W), np.uint8) if event == 3 else (np.arange(W * H).reshape(H, W) % 2).astype(np.uint8)
    h = _stack_hists(oracle, fr, sg, tss)
    a = oracle.Analyzer(fr, fr[0], sg, tss)
    start, rounds = 1, 0
    while True:
        st = a.find_trigger(start)
        for cls in (pyref.Sig, ts.HostSig):
            r = ts.ref_search(h, W * H, tss, start, sig_cls=cls)
            assert r["state"] == ts.DONE
            assert r["status"] == st["status"], (start, cls)
            if st["status"] == 0:
                assert r["trig"] == st["trig"]
            assert r["loc_thres"] in (-1, st["loc_thres"])
            assert (r["loc_thres"] == -1) == (r["evaluated"] == 0)
            tr = a.sig_trace()
            for i, v in r["main"].items():
                assert v == tr[i] or (math.isnan(v) and math.isnan(tr[i])), (i, v, tr[i])
        rounds += 1
        if st["status"] != 0:
            break
        start = st["trig"] + 1
    a.close()
    assert rounds >= 1


def test_reference_model_laziness_and_bad_frames():
    P, F = 1280 * 96, 41
    h = ts.step_stack(5, F, 22, P)
    full = ts.ref_search(h, P, 10)
    assert (full["state"], full["status"], full["trig"]) == (ts.DONE, 0, 22)
    cov = np.zeros(F, bool)
    cov[1:24] = True
    r = ts.ref_search(h, P, 10, covered=cov)
    assert (r["state"], r["need_frame"]) == (ts.NEED_FRAMES, 24)
    pend = np.zeros(F, bool)
    pend[23] = True
    r = ts.ref_search(h, P, 10, pending=pend)
    assert (r["state"], r["need_frame"]) == (ts.NEED_FINAL, 23)
    pend[:] = False
    pend[30] = True
    assert ts.ref_search(h, P, 10, pending=pend)["state"] == ts.DONE
    r = ts.ref_search(h, P, 10, first_bad=23)
    assert r["state"] == ts.BAD_LOOKAHEAD
    r = ts.ref_search(h, P, 10, first_bad=7)
    assert (r["state"], r["status"], r["evaluated"]) == (ts.DONE, -9, 6) and r["loc_thres"] >= 2
    r = ts.ref_search(h, P, 10, first_bad=1)
    assert (r["status"], r["loc_thres"]) == (-9, -1)
    assert ts.ref_search(h[:4], P, 10)["status"] == -9


def test_edge_scenes_hold_what_they_promise():
    """on the reference side: the arithmetic-edge set evaluates at least 20 NaN and 5 infinite values, and pyref.Sig and
    the host's significance agree on every one of them bit for bit"""
    nan = inf = 0
    for c in ts.edge_cases():
        t1, t2 = [], []
        r1 = ts.ref_of(c, pyref.Sig, t1)
        r2 = ts.ref_of(c, ts.HostSig, t2)
        assert ts.same_result(r1, r2)
        assert len(t1) == len(t2)
        for (i, n0, st, v), (_, _, _, w) in zip(t1, t2):
            assert v == w or (math.isnan(v) and math.isnan(w)), (i, n0, st, v, w)
            nan += math.isnan(v)
            inf += math.isinf(v)
    assert nan >= 20 and inf >= 5, (nan, inf)


def _limit():
    mf = C.c_int(0)
    assert _lib.lib().abub_trigger_search_limits(C.byref(mf), None) == 0
    return mf.value


@pytest.fixture(scope="module")
def designed():
    """the designed sets of trigscenes.py with the host model's result and trace of every case -- computed once"""
    sets = dict(seam=ts.seam_cases(limit=_limit()), chunk=ts.chunk_cases(limit=_limit()),
                edge=[c for F in (70, 131) for c in ts.edge_cases(F=F)], large=ts.large_p_cases())
    out = {}
    for name, cases in sets.items():
        refs = []
        for c in cases:
            tr = []
            refs.append((ts.ref_of(c, ts.HostSig, tr), tr))
        out[name] = (cases, refs)
    return out


def test_seam_scenes_hold_what_they_promise(designed):
    """what keeps the GPU tests of the seam scenes from passing vacuously, per seam s: both look-aheads evaluated across
    the seam (frame s + 1 against histories s and s - 1, frame s + 2 against s), a trigger at each of s - 1, s, s + 1,
    NEED_FRAMES / NEED_FINAL / BAD_LOOKAHEAD at s + 1 or s + 2 out of a look-ahead and NEED_* at s out of the main loop,
    -9 at the seam, a retry from s or s + 1 over three frames and more, a hole in a retry's history"""
    cases, refs = designed["seam"]
    limit = _limit()
    for F, s in ts.seam_sets(limit):
        mine = [(c, r, tr) for c, (r, tr) in zip(cases, refs) if len(c["hists"]) == F and c["seam"] == s]
        ev = {(i, n0, st) for _, _, tr in mine for i, n0, st, _ in tr}
        for want in ((s + 1, s, False), (s + 1, s - 1, False), (s + 2, s, False)):
            assert want in ev, (F, s, want)
        # (a trigger is decided at the second look-ahead: frame t can be one only where t + 2 is a frame)
        assert {t for t in (s - 1, s, s + 1) if t + 2 < F} <= {r["trig"] for _, r, _ in mine if r["status"] == 0}, (F, s)
        ahead, main = set(), set()
        for c, r, _ in mine:
            if c["what"] in ("step", "spike") and c["t0"] + 2 < F:
                assert (r["state"], r["status"], r["trig"]) == (ts.DONE, 0, c["t0"]), (F, s, c["t0"], r)  # where it was built to
            if r["state"] == ts.DONE:
                continue
            # the same search with nothing missing: how it first reads the frame this one stopped at
            ftr = []
            ts.ref_of(dict(c, covered=None, pending=None, first_bad=F), None, ftr)
            frame = c["first_bad"] if r["state"] == ts.BAD_LOOKAHEAD else r["need_frame"]
            first = [st for i, _, st, _ in ftr if i == frame][:1]
            if first == [False] and frame in (s + 1, s + 2):
                ahead.add(r["state"])
            elif first == [True] and frame in (s, s + 1, s + 2):
                main.add(r["state"])
        assert ahead == {ts.NEED_FRAMES, ts.NEED_FINAL, ts.BAD_LOOKAHEAD}, (F, s, ahead)
        assert main == {ts.NEED_FRAMES, ts.NEED_FINAL}, (F, s, main)
        assert any(c["what"] == "first_bad" and c["first_bad"] == s and (r["state"], r["status"]) == (ts.DONE, -9) for c, r, _ in mine)
        assert any(c["start"] in (s, s + 1) and r["state"] == ts.DONE and r["evaluated"] >= 3 for c, r, _ in mine), (F, s)
        assert any(c["what"] == "hole below start" and (r["state"], r["need_frame"]) == (ts.NEED_FRAMES, 10) for c, r, _ in mine)
        assert {c["tss"] for c, _, _ in mine} == {2, 10}
    _, ms = C.c_int(0), C.c_int(0)
    _lib.lib().abub_trigger_search_limits(None, C.byref(ms))
    assert max(len(ts.segments_of(c)) for c in cases if len(c["hists"]) == limit) == min(ms.value, (limit + 15) // 16)


def _top(row):
    return int(np.flatnonzero(row)[-1])


def test_chunk_scenes_hold_what_they_promise(designed):
    """the last bin a stored frame pushes takes every value around the kernel's 64-bin chunks; look-aheads behind the
    first tile run over bins >= 64; the scenes have the shapes their names say"""
    cases, refs = designed["chunk"]
    last, high = set(), 0
    for c, (r, tr) in zip(cases, refs):
        for i, n0, st, v in tr:
            lb = ts.walk(c["hists"][i], c["P"])[0]
            if st:
                last.add(lb)
            elif i > 64 and lb >= 64:
                high += 1
    assert last >= {63, 64, 127, 128, 191, 192, 255}, sorted(last)
    assert high >= 3, high
    assert {len(c["hists"]) for c in cases} == {70, 131, _limit()}
    assert set(ts.CHUNK_TOPS) <= {_top(c["hists"][i]) for c in cases for i in range(1, len(c["hists"]))}
    for c in cases:
        h, s = c["hists"], c["seam"]
        if c["what"] == "low tile between high ones":
            assert max(_top(r) for r in h[1:65]) >= 200 and max(_top(r) for r in h[65:129]) < 10 and _top(h[129]) >= 200
        elif c["what"] == "lane 63 low":
            assert _top(h[s]) + 100 <= min(_top(h[s - 1]), _top(h[s + 1]))
        elif c["what"] == "lane 63 high":
            assert _top(h[s]) >= 100 + max(_top(h[s - 1]), _top(h[s + 1]))
    assert {"low tile between high ones", "lane 63 low", "lane 63 high"} <= {c["what"] for c in cases}
    stale = [(r, tr) for c, (r, tr) in zip(cases, refs) if c["what"] == "previous tile's last frame pushed nothing"]
    assert len(stale) == 2
    for r, tr in stale:  # the flicker at 127 reaches its second look-ahead, frame 129 in tile 2, and fails there
        v = [v for i, n0, st, v in tr if (i, n0, st) == (129, 127, False)]
        assert len(v) == 1 and v[0] < 3 and (r["state"], r["status"]) == (ts.DONE, -3), (v, r)


def test_seam_edge_scenes_hold_what_they_promise(designed):
    """NaN and infinite values among the evaluations behind the first tile, with the histories that made them carried
    over the seam"""
    cases, refs = designed["edge"]
    vals = [v for _, (_, tr) in zip(cases, refs) for i, _, _, v in tr if i > 64]
    nan, inf = sum(math.isnan(v) for v in vals), sum(math.isinf(v) for v in vals)
    assert nan >= 10 and inf >= 3, (nan, inf)


def test_large_p_scenes_hold_what_they_promise(designed):
    """above 2^24 pixels the reference's float counter departs from the exact one: it ends one short (the last non-zero
    bin is dropped), one over (the walk runs to bin 255), and a count above 2^24 is pushed rounded; one stack triggers"""
    cases, refs = designed["large"]
    short = over = rounded = 0
    for c, (r, tr) in zip(cases, refs):
        for i, n0, st, v in tr:
            row = c["hists"][i]
            lb, rem, ex = ts.walk(row, c["P"])
            short += lb < _top(row) and rem == 0 and ex == 1
            over += lb == 255 and _top(row) < 255 and rem == 1 and ex == 0
            rounded += st and any(int(np.float32(row[b])) != int(row[b]) for b in range(1, lb + 1))
    assert short >= 1 and over >= 1 and rounded >= 1, (short, over, rounded)
    assert sum(r["status"] == 0 for r, _ in refs) >= 1
    assert {c["P"] for c in cases} == {(1 << 24) + 1, 4097 * 4097, (1 << 24) + 2, _lib.TRIG_MAX_PIXELS}
    assert {len(c["hists"]) for c in cases} == {12, 70}


def test_both_models_agree_on_the_designed_scenes(designed):
    """pyref.Sig and the host's significance on every case of the four designed sets: fields, main values and the trace
    as bit patterns.  Of the stacks at the frame limit only the step stacks run through pyref.Sig too (it re-sums the
    whole history for every bin: seconds per such stack); the others of that length are the host model's alone."""
    limit = _limit()
    n = 0
    for name, (cases, refs) in designed.items():
        for c, (r2, t2) in zip(cases, refs):
            if len(c["hists"]) == limit and c["what"] != "step":
                continue
            t1 = []
            r1 = ts.ref_of(c, pyref.Sig, t1)
            assert ts.same_result(r1, r2), (name, c.get("what"), r1, r2)
            assert len(t1) == len(t2) and r1["main"].keys() == r2["main"].keys()
            for (i, n0, st, v), (i2, n2, st2, w) in zip(t1, t2):
                assert (i, n0, st) == (i2, n2, st2)
                assert v == w or (math.isnan(v) and math.isnan(w)), (name, c.get("what"), i, n0, st, v, w)
            n += 1
    assert n >= 200


def test_new_entries_declared_exported_and_bound():
    from autobub3hs_amd import hip

    hdr = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = C.CDLL(_lib.build())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
        before = hdr[:hdr.index(name + "(")]
        assert "AnalyzerUnit.cpp:119-324, 435-504, 514-532" in before[before.rindex("/*"):].replace("\n *", ""), name
    for rec, size in ((_lib.TrigSeg, 24), (_lib.TrigStack, 24)):
        assert C.sizeof(rec) == size
    for word in ("abub_trig_seg", "abub_trig_stack", "abub_trig_result", "ABUB_TRIG_NEED_FINAL", "ABUB_TRIG_BAD_LOOKAHEAD"):
        assert word in txt, word
    assert callable(hip.trigger_search) and callable(hip.trigger_search_limits)
    assert "abh_pipe_trigger_stats" in host.SIGNATURES and callable(host.Pipeline.trigger_stats)


def test_limits_and_sizes_need_no_device():
    lib = _lib.lib()
    mf, ms = C.c_int(-1), C.c_int(-1)
    assert lib.abub_trigger_search_limits(C.byref(mf), C.byref(ms)) == 0
    assert mf.value >= 64 and ms.value >= 32
    assert lib.abub_trigger_search_limits(None, None) == 0
    assert lib.abub_trigger_search_desc_bytes(4, 9) >= 4 * 24 + 9 * 24
    assert lib.abub_trigger_search_desc_bytes(0, 0) == 0 and lib.abub_trigger_search_desc_bytes(-1, 3) == 0


def test_trigger_search_refuses_bad_arguments_before_the_device():
    lib = _lib.lib()
    mf, ms = C.c_int(0), C.c_int(0)
    lib.abub_trigger_search_limits(C.byref(mf), C.byref(ms))
    one = C.c_void_p(256)  # never dereferenced: every call below is refused while the arguments are checked
    st = (_lib.TrigStack * 2)()
    sg = (_lib.TrigSeg * 2)()
    for k in range(2):
        st[k].seg0, st[k].nseg, st[k].F, st[k].start, st[k].tss, st[k].first_bad = k, 1, 41, 1, 10, 41
        sg[k].hist, sg[k].pending, sg[k].first, sg[k].count = 256, None, 1, 40
    S, G = C.addressof(st), C.addressof(sg)
    # (stacks, segs, nstacks, nsegs, W, H, desc, desc_bytes, out, sig_main, sig_pitch, stream)
    good = [S, G, 2, 2, 64, 48, one, 1 << 16, one, None, 0, None]
    for pos, bad in ((0, None), (1, None), (6, None), (8, None), (2, -1), (3, -1), (4, 0), (5, 0), (4, 1 << 16)):
        args = list(good)
        args[pos] = bad
        if pos == 4 and bad == 1 << 16:
            args[5] = 1 << 16  # W * H beyond int
        assert lib.abub_trigger_search_dev(*args) == -1, pos
        assert b"bad arguments" in lib.abub_last_error(), pos
    # W * H within int, but above the largest pixel count whose float stays below 2^31: refused by name; the bound itself
    # passes the check (and is refused for the next thing wrong, here the scratch size)
    wide = _lib.TRIG_MAX_PIXELS
    assert wide == 2 ** 31 - 65 and np.float32(wide) == 2.0 ** 31 - 128 and np.float32(wide + 1) == 2.0 ** 31
    for w, h in ((wide + 1, 1), (2 ** 31 - 1, 1), (33554431, 64), (2, 1073741823)):
        args = list(good)
        args[4], args[5] = w, h
        assert lib.abub_trigger_search_dev(*args) == -1, (w, h)
        assert b"ABUB_TRIG_MAX_PIXELS" in lib.abub_last_error(), (w, h)
    for w, h in ((wide, 1), (1, wide), (715827861, 3), (46340, 46340)):
        args = list(good)
        args[4], args[5], args[7] = w, h, 8
        assert lib.abub_trigger_search_dev(*args) == -1 and b"scratch" in lib.abub_last_error(), (w, h)
    args = list(good)
    args[2] = 0
    args[4], args[5] = wide, 1
    assert lib.abub_trigger_search_dev(*args) == 0  # the bound, and nothing to do
    args = list(good)
    args[9], args[10] = one, 0  # sig_main without a pitch
    assert lib.abub_trigger_search_dev(*args) == -1
    args[10] = 40  # ... or with one below F
    assert lib.abub_trigger_search_dev(*args) == -1
    args = list(good)
    args[7] = 8
    assert lib.abub_trigger_search_dev(*args) == -1 and b"scratch" in lib.abub_last_error()
    args = list(good)
    args[6] = C.c_void_p(264)
    assert lib.abub_trigger_search_dev(*args) == -1 and b"scratch" in lib.abub_last_error()
    # a stack beyond either limit, a descriptor outside the segment array, overlapping segments
    st[1].F = mf.value + 1
    assert lib.abub_trigger_search_dev(*good) == -1 and b"more frames" in lib.abub_last_error()
    st[1].F = 41
    st[1].nseg = ms.value + 1
    assert lib.abub_trigger_search_dev(*good) == -1 and b"more segments" in lib.abub_last_error()
    st[1].nseg = 2
    assert lib.abub_trigger_search_dev(*good) == -1 and b"descriptor" in lib.abub_last_error()
    st[1].seg0, st[1].nseg = 0, 2  # its two segments both start at frame 1
    assert lib.abub_trigger_search_dev(*good) == -1 and b"overlap" in lib.abub_last_error()
    sg[1].first = 41
    sg[1].hist = None
    assert lib.abub_trigger_search_dev(*good) == -1 and b"overlap" in lib.abub_last_error()
    assert lib.abub_trigger_search_dev(S, G, 0, 0, 64, 48, one, 0, one, None, 0, None) == 0  # nothing to do
    assert lib.abub_trigger_clear_pending_dev(None, one, 4, None) == -1 and lib.abub_trigger_clear_pending_dev(one, None, 4, None) == -1
    assert lib.abub_trigger_clear_pending_dev(one, one, 0, None) == 0


def test_pipeline_option_trigger_is_known_and_validated():
    L = host.lib()
    L.abh_pipe_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.abh_pipe_error.restype = C.c_char_p
    assert L.abh_pipe_set_option(None, b"trigger", 1) == -1  # valid name and value, but no pipeline
    assert b"no pipeline" in L.abh_pipe_error()
    assert b"unknown option" not in L.abh_pipe_error()
    for v in (-1, 2):
        assert L.abh_pipe_set_option(None, b"trigger", v) == -1
        assert b"0 or 1" in L.abh_pipe_error()
