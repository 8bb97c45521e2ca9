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


def step_stack(seed, F, t0, P, flicker=None):
    """a quiet stack with a bubble that starts at t0 and grows (and optionally a one-frame flicker before it)"""
    rng = np.random.RandomState(seed)
    h = _noise(rng, F, 0.5)
    for i in range(t0, F):
        h[i, 2:30] += 60 + 30 * (i - t0)
    if flicker is not None:
        h[flicker, 2:7] += 400
    h[:, 0] = 0
    h[:, 0] = P - h.sum(1)
    h[0] = 0
    return h.astype(np.uint32)


def edge_cases(P=512 * 512, F=12):
    """Arithmetic edges: wrapped squares (negative variance -> NaN), constant columns (sd = 0, term skipped), a constant
    history with a different look-ahead count (+-inf, then inf - inf), and frames that stop below earlier frames' bins."""
    rng = np.random.RandomState(11)
    cases = []

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
        tj = 3 + k % 5
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
        h[6 + k % 3:, 2:5] += 900
        fin(h, (2, 10)[k % 2])
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
