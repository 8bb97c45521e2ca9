"""Scenes and the reference model for the device trigger search (K6, abub_trigger.hip).

ref_search() is AnalyzerUnit::FindTriggerFrame (AnalyzerUnit.cpp:119-324) driven by histograms instead of frames, on
top of a stateful significance object: pyref.Sig (pure Python, the CPU tests check it against the oracle) or HostSig
(host/hostlogic.cpp significanceFromHist through host.Significance: the same state machine, fast enough for hundreds of
stacks).  A retry (start > 1) replays frames 1 .. start - 1 with store = True first: that is the history the analyzer
holds when FindTriggerFrame is called again behind a trigger.  Laziness follows the kernel's contract: the first frame
the search touches (history first) that is not covered gives NEED_FRAMES, a covered but pending one NEED_FINAL.
"""
import numpy as np

import pyref

DONE, NEED_FRAMES, NEED_FINAL, BAD_LOOKAHEAD = 0, 1, 2, 3
FIELDS = ("state", "status", "trig", "loc_thres", "need_frame", "evaluated")


class HostSig:
    """host.Significance with pyref.Sig's interface"""

    def __init__(self, P, tss):
        from autobub3hs_amd import host
        self.s, self.P = host.Significance(tss), P

    def __call__(self, h, store):
        return self.s(h, self.P, store)

    @property
    def loc_thres(self):
        return self.s.loc_thres.value


def ref_search(hists, P, tss, start=1, first_bad=None, covered=None, pending=None, sig_cls=pyref.Sig, trace=None):
    """-> dict of the fields of abub_trig_result.  hists: [F][256] (row 0 unused).  trace (a list) receives
    (frame, history length, store, value) of every evaluation of the search itself (not of the replay)."""
    n = len(hists)
    first_bad = n if first_bad is None else first_bad
    covered = np.ones(n, bool) if covered is None else covered
    pending = np.zeros(n, bool) if pending is None else pending
    res = dict(state=DONE, status=-3, trig=0, loc_thres=-1, need_frame=0, evaluated=0, sig=0.0, main={})
    if n < 5:
        res["status"] = -9
        return res
    f32 = np.float32
    thr = f32(3.5)
    if tss < 6:
        thr = f32(float(thr) * (5 / 3.5))
    start = max(start, 1)

    def need(i):
        return dict(state=NEED_FINAL if covered[i] else NEED_FRAMES, status=-3, trig=0, loc_thres=-1, need_frame=i,
                    evaluated=0, sig=0.0, main={})

    def readable(i):
        return covered[i] and not pending[i]

    sig = sig_cls(P, tss)
    for i in range(1, min(start, n)):
        if i >= first_bad:
            break
        if not readable(i):
            return need(i)
        sig(hists[i], True)
    for i in range(start, n):
        if i >= first_bad:
            res["status"] = -9
            return res
        if not readable(i):
            return need(i)
        v = sig(hists[i], True)
        if trace is not None:
            trace.append((i, i, True, v))
        s = f32(v)
        res["main"][i] = v
        res["loc_thres"] = sig.loc_thres
        res["sig"] = float(s)
        res["evaluated"] += 1
        if s > thr and i >= 2 and i != n - 1:
            mx = float(s)
            for ii in (1, 2):
                if i + ii >= n:
                    break
                if i + ii >= first_bad:
                    res["state"] = BAD_LOOKAHEAD
                    return res
                if not readable(i + ii):
                    return need(i + ii)
                v = sig(hists[i + ii], False)
                if trace is not None:
                    trace.append((i + ii, i, False, v))
                s = f32(v)
                with np.errstate(all="ignore"):
                    val = np.float64(s) / (np.float64(thr) / 3.5 * 5) + np.float64(s) / np.float64(mx)
                if val <= 3:
                    break
                elif ii == 2:
                    res["status"], res["trig"] = 0, i
                if float(s) > mx:
                    mx = float(s)
            if res["status"] == 0:
                return res
    return res


def same_result(dev, ref):
    """the device's result dict against the model's: every integer field, and the float bit for bit (NaN == NaN)"""
    for k in FIELDS:
        if dev[k] != ref[k]:
            return False
    a, b = np.float32(dev["sig"]), np.float32(ref["sig"])
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


# ---- synthetic histogram stacks --------------------------------------------------------------------------------------
KINDS = ("quiet", "step", "flicker1", "flicker2", "late")


def _noise(rng, F, scale=1.0):
    """what D(i; i - off) leaves of sensor noise behind the 6 sigma cut: a few pixels in the lowest bins"""
    h = np.zeros((F, 256), np.int64)
    lam = 120.0 * scale * np.exp(-np.arange(1, 9) / 1.6)
    h[:, 1:9] = rng.poisson(lam, (F, 8))
    return h


def random_stack(rng, F, kind, P):
    """[F][256] uint32 histograms (row 0 zero but for bin 0) of one stack of the given kind, each row summing to P"""
    h = _noise(rng, F)
    t0 = None
    if kind in ("step", "late") and F >= 5:
        t0 = int(rng.randint(2, max(3, F - 3))) if kind == "step" else int(rng.randint(max(2, F - 2), F))
        for i in range(t0, F):
            k = i - t0
            top = int(rng.randint(12, 60))
            amp = 40 + 25 * min(k, 20)
            h[i, 2:top] += rng.poisson(amp * np.exp(-np.arange(top - 2) / (0.3 * top)))
    elif kind in ("flicker1", "flicker2") and F >= 7:
        tf = int(rng.randint(2, F - 3))
        for i in range(tf, min(F, tf + (1 if kind == "flicker1" else 2))):
            h[i, 2:7] += rng.poisson(400, 5)
    h[:, 0] = 0
    h[:, 0] = P - h.sum(1)
    assert (h[:, 0] >= 0).all()
    h[0] = 0
    return h.astype(np.uint32), t0


def random_cases(seed, n, frame_counts, P):
    """n stacks over every kind, frame count and tss in turn (so each combination appears), fully covered"""
    rng = np.random.RandomState(seed)
    cases = []
    for k in range(n):
        F = frame_counts[k % len(frame_counts)]
        kind = KINDS[(k // len(frame_counts)) % len(KINDS)]
        tss = (2, 10)[(k // 3) % 2]
        h, _ = random_stack(rng, F, kind, P)
        # fully covered, in one to three adjoining segments
        cuts = sorted(set(int(c) for c in rng.randint(2, max(3, F), int(rng.randint(0, 3))) if 1 < c < F))
        cases.append(dict(hists=h, P=P, tss=tss, start=1, first_bad=F, cuts=cuts, kind=kind))
    return cases


def step_stack(seed, F, t0, P, flicker=None, flicker_len=1):
    """a quiet stack with a bubble that starts at t0 and grows (t0 = F: none), and optionally a flicker of one frame, or
    of flicker_len frames, from frame `flicker` on"""
    rng = np.random.RandomState(seed)
    h = _noise(rng, F, 0.5)
    for i in range(t0, F):
        h[i, 2:30] += 60 + 30 * (i - t0)
    if flicker is not None:
        h[flicker:flicker + flicker_len, 2:7] += 400
    h[:, 0] = 0
    h[:, 0] = P - h.sum(1)
    h[0] = 0
    return h.astype(np.uint32)


def spike_stack(seed, F, t0, P):
    """a small bubble from t0 on (bins 2 .. 6 only) with one very bright frame at t0 + 1.  The search triggers at t0 on
    its second look-ahead, frame t0 + 2, whose history is frames 1 .. t0: were frame t0 + 1 left in that history, its
    standard deviations would be some hundred times larger and the look-ahead would fail."""
    rng = np.random.RandomState(seed)
    h = _noise(rng, F, 0.5)
    h[t0:, 2:7] += 30
    h[t0 + 1, 2:7] += 4000
    h[:, 0] = 0
    h[:, 0] = P - h.sum(1)
    h[0] = 0
    return h.astype(np.uint32)


def seams_of(F):
    """the kernel's tile seams of an F-frame stack: s with frames s | s + 1 in different 64-frame tiles (tiles start at 1)"""
    return range(64, F - 1, 64)


def edge_cases(P=512 * 512, F=12):
    """Arithmetic edges: wrapped squares (negative variance -> NaN), constant columns (sd = 0, term skipped), a constant
    history with a different look-ahead count (+-inf, then inf - inf), and frames that stop below earlier frames' bins.
    With F > 64 (70, 131) the jumps and the changes of the constant columns sit at s - 1 .. s + 2 of a tile seam s (64, 128)
    of the kernel, so NaN, +-inf and a negative sum of squares are history carried from one tile into the next."""
    rng = np.random.RandomState(11)
    cases = []
    seams = list(seams_of(F))

    def at(k, short):
        """where family member k's event starts: as ever in a short stack, else at s - 1 .. s + 2 of the seams in turn"""
        return short if not seams else seams[k % len(seams)] - 1 + (k // len(seams)) % 4

    def fin(h, tss):
        h[:, 0] = 0
        h[:, 0] = P - h.sum(1)
        assert (h[:, 0] >= 0).all()
        h[0] = 0
        cases.append(dict(hists=h.astype(np.uint32), P=P, tss=tss, start=1, first_bad=F, cuts=[]))

    for k in range(8):  # counts in 46341 .. 60000: the int square wraps, S2 may go negative
        h = np.zeros((F, 256), np.int64)
        nb = 2 + k % 3
        h[:, 2:2 + nb] = rng.randint(46341, 60001, (F, nb))
        if k % 2:
            h[:, 9] = rng.randint(0, 50, F)
        fin(h, (2, 10)[k % 2])
    for k in range(10):  # constant columns, a jump in a varying one, then look-ahead frames that differ in the constant ones
        h = np.zeros((F, 256), np.int64)
        h[:, 3] = 100
        h[:, 4] = 50
        h[:, 6:13] = 10 + rng.randint(0, 3, (F, 7))
        tj = at(k, 3 + k % 5)
        h[tj:, 6:13] += 3000
        if k < 5:
            h[tj + 1:, 3] = 200 + k      # only upwards: +inf and stays there
        else:
            h[tj + 1:, 3] = 200 + k      # +inf ...
            h[tj + 1:, 4] = 20           # ... then -inf: inf - inf
        fin(h, (2, 10)[k % 2])
    for k in range(6):  # early frames reach high bins, later frames stop far below them
        h = np.zeros((F, 256), np.int64)
        h[1:4, 2:200] = rng.randint(0, 40, (3, 198))
        h[4:, 2:6] = rng.randint(0, 40, (F - 4, 4))
        h[at(k, 6 + k % 3):, 2:5] += 900
        fin(h, (2, 10)[k % 2])
    return cases


def walk(h, P):
    """one evaluation's way through the bins of histogram h with the reference's counter (`pix_rem -= binEntry`, an int
    -= float, AnalyzerUnit.cpp:493) -> (last bin walked, the counter behind it, the exact counter behind it)"""
    rem = ex = int(P)
    last = 0
    for i in range(256):
        if rem <= 0:
            break
        last = i
        rem = int(np.float32(rem) - np.float32(h[i]))
        ex -= int(h[i])
    return last, rem, ex


def _fin(h, P):
    h[:, 0] = 0
    h[:, 0] = P - h.sum(1)
    assert (h[:, 0] >= 0).all()
    h[0] = 0
    return h.astype(np.uint32)


def _case(h, P, tss, what, **kw):
    c = dict(hists=h, P=P, tss=tss, start=1, first_bad=len(h), cuts=[], what=what)
    c.update(kw)
    return c


def seam_sets(limit=512):
    """(F, s): the frame counts of the designed scenes and the tile seam the scene is built around"""
    assert limit > 130
    return (67, 64), (70, 64), (131, 64), (131, 128), (limit, max(seams_of(limit)))


# step stacks whose first seed has a noise frame just below t0 that passes both look-aheads and triggers in its place
_SEAM_RESEED = {(131, 128, 128): 1, (512, 448, 449): 1}
_SPIKE_RESEED = {(67, 64, 64): 4, (512, 448, 448): 1}


def seam_cases(P=1280 * 96, limit=512):
    """Decisions placed at a tile seam s of the kernel (frames s | s + 1 lie in different 64-frame tiles).  Per (F, s) of
    seam_sets(): a growing step (step_stack: it triggers at t0) and a one- and a two-frame flicker (a look-ahead that
    fails) at each of s - 2 .. s + 2, a spike_stack at s - 2 .. s (its second look-ahead decides by the history alone), and on the step stacks retries from s .. s + 2 and from behind the trigger,
    first_bad, the end of the coverage and a pending frame at s .. s + 2, a hole in the history of a retry, and segment
    cuts at the seam and every 16 frames.  Each case says in `what`, `seam` and `t0` what it was built as."""
    cases = []
    for n, (F, s) in enumerate(seam_sets(limit)):
        steps = {}
        for k, t0 in enumerate(range(s - 2, s + 3)):
            tss = (2, 10)[(k + n) % 2]
            h = step_stack(7000 + 100 * n + t0 + 1000 * _SEAM_RESEED.get((F, s, t0), 0), F, t0, P)
            steps[t0] = (h, tss)
            cases.append(_case(h, P, tss, "step", seam=s, t0=t0))
            for fl in (1, 2):  # the flicker at t0, and (where there is room) a bubble some frames behind it
                hf = step_stack(7050 + 100 * n + 10 * fl + t0, F, t0 + 8 if t0 + 12 < F else F, P, t0, fl)
                cases.append(_case(hf, P, (10, 2)[(k + n) % 2], "flicker%d" % fl, seam=s, t0=t0))
        for k, t0 in enumerate((s - 2, s - 1, s)):  # the second look-ahead is frame s, s + 1 (lane 0 of the next tile), s + 2
            cases.append(_case(spike_stack(7090 + 100 * n + t0 + 1000 * _SPIKE_RESEED.get((F, s, t0), 0), F, t0, P), P, (10, 2)[(k + n) % 2], "spike", seam=s, t0=t0))
        for t0 in (s - 1, s, s + 1, s + 2):
            h, tss = steps[t0]
            kw = dict(seam=s, t0=t0)
            if t0 in (s, s + 2):
                for st in (s, s + 1, s + 2):
                    cases.append(_case(h, P, tss, "retry", start=st, **kw))
            if t0 <= s + 1:
                cases.append(_case(h, P, tss, "retry behind the trigger", start=t0 + 1, **kw))
                for fb in (s, s + 1, s + 2):
                    cases.append(_case(h, P, tss, "first_bad", first_bad=fb, **kw))
            if t0 in (s, s + 2):  # NEED_* from the look-aheads of main frame s, and from the main loop
                for e in (s - 1, s, s + 1):
                    cov = np.zeros(F, bool)
                    cov[1:e + 1] = True
                    cases.append(_case(h, P, tss, "covered", covered=cov, pending=np.zeros(F, bool), end=e, **kw))
                    pend = np.zeros(F, bool)
                    pend[e + 1] = True
                    cases.append(_case(h, P, tss, "pending", covered=np.ones(F, bool), pending=pend, **kw))
        h, tss = steps[s + 1]
        cov = np.ones(F, bool)
        cov[10] = False  # a frame of the history of a retry, one tile (or more) below it
        cases.append(_case(h, P, tss, "hole below start", start=s + 2, covered=cov, pending=np.zeros(F, bool), seam=s, t0=s + 1))
        cases.append(_case(h, P, tss, "cuts at the seam", cuts=[s, s + 1], seam=s, t0=s + 1))
        h, tss = steps[s]
        cases.append(_case(h, P, tss, "cuts every 16", cuts=list(range(16, F, 16)), seam=s, t0=s))
    return cases


CHUNK_TOPS = (63, 64, 65, 127, 128, 129, 191, 192, 255)


def _chunk_stack(rng, F, P, tops, change=None):
    """counts up to bin tops[i] in frame i: a level per bin plus a unit that alternates along the bins and the frames, so a
    frame's terms cancel in pairs and only what `change` adds (or a frame that pushes bins others did not) is significant"""
    level = rng.randint(3, 40, 256)
    i, b = np.meshgrid(np.arange(F), np.arange(256), indexing="ij")
    h = (level[None, :] + ((i + b) & 1)).astype(np.int64)
    if change is not None:
        change(h)
    h[:, :2] = 0
    h[b > np.asarray(tops)[:, None]] = 0
    return _fin(h, P)


def chunk_cases(P=1280 * 96, limit=512):
    """Stacks longer than a tile whose frames push counts beyond the first 64-bin chunk the kernel stages, up to bin 255:
    the prefix sums of bins >= 64 are carried over a seam, a tile that ends in chunk 0 lies between two that reach bin
    220, frame s (lane 63 of its tile) stops 130 bins below or above its neighbours, and steps and flickers in the high
    bins at s - 1 .. s + 1 make the look-aheads run over those bins across the seam."""
    rng = np.random.RandomState(23)
    cases = []

    def step(t0, lo, hi, grow=15):
        def f(h):
            for i in range(t0, len(h)):
                h[i, lo:hi + 1] += 40 + grow * (i - t0)
        return f

    def flicker(t0, n, lo, hi):
        def f(h):
            h[t0:t0 + n, lo:hi + 1] += 150
        return f

    sets = [(70, 64), (131, 64), (131, 128), (limit, max(seams_of(limit)))]
    for n, (F, s) in enumerate(sets):
        tss = (10, 2)[n % 2]
        tops = [255] * F  # every CHUNK_TOPS value as a frame's last bin, at s - 6 .. s + 2
        tops[s - 6:s + 3] = CHUNK_TOPS if n % 2 == 0 else CHUNK_TOPS[::-1]
        cases.append(_case(_chunk_stack(rng, F, P, tops), P, tss, "tops", seam=s))
        if F == limit:
            break  # (one case at the limit)
        tops = [230] * F
        tops[s] = 100
        cases.append(_case(_chunk_stack(rng, F, P, tops, step(s - 1, 150, 200)), P, tss, "lane 63 low", seam=s))
        tops = [100] * F
        tops[s] = 230
        cases.append(_case(_chunk_stack(rng, F, P, tops, flicker(s - 1, 2, 60, 100)), P, 12 - tss, "lane 63 high", seam=s))
        for t0 in (s, s + 1):
            cases.append(_case(_chunk_stack(rng, F, P, [255] * F, step(t0, 192, 255)), P, (2, 10)[t0 % 2], "high step", seam=s, t0=t0))
        cases.append(_case(_chunk_stack(rng, F, P, [255] * F, flicker(s, 1, 100, 255)), P, tss, "high flicker", seam=s))
        if F == 131 and s == 64:
            tops = [220] * 65 + [8] * 64 + [220] * 2  # tile 1 never leaves chunk 0: every chunk after the first is skipped
            cases.append(_case(_chunk_stack(rng, F, P, tops), P, tss, "low tile between high ones", seam=s))
            # The same, with a second look-ahead that decides by what tile 1's last frame pushed in the high bins: nothing.
            # Frame 64 (the last of tile 0) holds 30000 in bin 200; a flicker at 127, 128 passes its first look-ahead; the
            # second one, frame 129 against history 127, has 3000 in bin 200 and zeros below it.  With frame 64 in that
            # history its term is about 1 and the look-ahead fails; a history that has lost frame 64 (its count taken off
            # once more as "frame 128's") makes it some hundreds, a trigger at 127.
            def stale(h):
                h[64, 200] = 30000
                h[127:129, 2:7] += 400
                h[129:, 7:200] = 0
                h[129:, 200] = 3000
            tops = [220] * 65 + [8] * 64 + [200] * 2
            for t in (10, 2):
                cases.append(_case(_chunk_stack(rng, F, P, tops, stale), P, t, "previous tile's last frame pushed nothing", seam=128))
    return cases


LARGE_P = ((16777217, 1), (4097, 4097), (8388609, 2), (2147483583, 1))  # 2^24 + 1, 4097^2, 2^24 + 2, the entry's bound


def large_p_cases():
    """P = W * H above 2^24, where the reference's float counter rounds: it ends one short of the exact one (the last
    non-zero bin, one pixel, is neither pushed nor summed) or one over (the walk runs to bin 255), and a bin count above
    2^24 is pushed rounded.  Each stack has a step, at F = 70 at the tile seam.  The cases carry their own W and H."""
    rng = np.random.RandomState(29)
    cases = []
    for n, (W, H) in enumerate(LARGE_P):
        P = W * H
        for F in (12, 70):
            t0 = F - 6  # 6, and 64: the seam
            for variant in ("odd rest", "one pixel", "big bin 1", "big bin 2"):
                h = np.zeros((F, 256), np.int64)
                if variant == "one pixel":
                    h[:, 5] = 1
                else:
                    h[:, 3:9] = rng.randint(5, 30, (F, 6))
                    h[:, 40] = rng.randint(1, 3, F)  # the last bin holds one pixel, or two: dropped, or pushed
                if variant.startswith("big bin"):  # in bin 1, which no term reads, or in bin 2 (NaN from there on)
                    if P < (1 << 24) + 8000:
                        continue  # (no bin but bin 0 can hold more than 2^24 there)
                    big = (1 << 24) + 1 if P < (1 << 30) + 8000 else (1 << 30) + 1
                    h[:, int(variant[-1])] = big + 2 * rng.randint(0, 2000, F)
                for i in range(t0, F):
                    h[i, 4:21] += 60 + 30 * (i - t0)
                h[:, 3] += 1 - h.sum(1) % 2  # an odd number of pixels outside bin 0
                tss = (2, 10)[(n + (F == 70)) % 2]
                cases.append(_case(_fin(h, P), P, tss, variant, W=W, H=H, t0=t0))
    return cases


def segments_of(case):
    """[(first, count)] of a case: from `covered` (maximal runs) or, for a fully covered stack, from its `cuts`"""
    F = len(case["hists"])
    cov = case.get("covered")
    if cov is None:
        edges = [1] + [c for c in case.get("cuts", []) if 1 < c < F] + [F]
        return [(a, b - a) for a, b in zip(edges[:-1], edges[1:]) if b > a]
    segs, i = [], 1
    while i < F:
        if cov[i]:
            j = i
            while j < F and cov[j]:
                j += 1
            segs.append((i, j - i))
            i = j
        else:
            i += 1
    return segs


def run_device(cases, W, H, order=None):
    """the cases through hip.trigger_search in one launch (optionally in another order) -> (results, sig_main numpy),
    both in the order of `cases`"""
    import torch

    from autobub3hs_amd import hip
    order = list(range(len(cases))) if order is None else list(order)
    rows, pend, at = [], [], []
    off = 0
    for k in order:
        at.append(off)
        h = cases[k]["hists"]
        rows.append(h)
        p = cases[k].get("pending")
        pend.append(np.zeros(len(h), np.uint8) if p is None else np.asarray(p, np.uint8))
        off += len(h)
    big = torch.from_numpy(np.concatenate(rows).astype(np.int64).astype(np.int32, casting="unsafe")).cuda()
    bigp = torch.from_numpy(np.concatenate(pend)).cuda()
    stacks = []
    for k, o in zip(order, at):
        c = cases[k]
        F = len(c["hists"])
        segs = [(a, big[o + a:o + a + n], bigp[o + a:o + a + n] if c.get("pending") is not None else None)
                for a, n in segments_of(c)]
        stacks.append(dict(F=F, tss=c["tss"], start=c.get("start", 1), first_bad=c.get("first_bad", F), segs=segs))
    res, sm = hip.trigger_search(stacks, W, H)
    sm = sm.cpu().numpy()
    out, outs = [None] * len(cases), [None] * len(cases)
    for pos, k in enumerate(order):
        out[k], outs[k] = res[pos], sm[pos]
    return out, outs


def ref_of(case, sig_cls=None, trace=None):
    return ref_search(case["hists"], case["P"], case["tss"], case.get("start", 1), case.get("first_bad"),
                      case.get("covered"), case.get("pending"), sig_cls or HostSig, trace)
