"""K7 (abub_localize.hip) alone, through hip.py.  K7a against the host's describe columns (the C-surface probe), every
column as a bit pattern; K7b against the contour-driven reference localizer of locscenes.py (checked on the CPU against the
oracle by test_localize_abi.py) on the hand-made stacks, with the lists' capacities one short, and behind K7a on random
polygons."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import locscenes as ls  # noqa: E402
from autobub3hs_amd import hip, host  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def dev(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype) if a.dtype != dtype else np.ascontiguousarray(a)).to(DEV)


def contour_list(slots):
    """slots: per slot a list of polygons (int32 [n, 2]), or None for a slot the tracer declined -> the dict
    hip.trace_contours() returns, as K5 leaves it (true offsets, x | y << 16)"""
    n = len(slots)
    status = np.array([0 if s is not None else 1 for s in slots], np.uint32)
    coff, poff = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32)
    npts, pts = [], []
    for i, s in enumerate(slots):
        for p in (s or []):
            npts.append(len(p))
            pts.append(p[:, 0].astype(np.uint32) | (p[:, 1].astype(np.uint32) << 16))
        coff[i + 1] = len(npts)
        poff[i + 1] = sum(npts)
    pts = np.concatenate(pts) if pts else np.zeros(0, np.uint32)
    pad = lambda a: np.concatenate([np.asarray(a, np.uint32), np.zeros(1, np.uint32)])
    return {"status": dev(status), "cont_off": dev(coff), "cont_npts": dev(pad(npts)), "pt_off": dev(poff), "pts": dev(pad(pts)),
            "ncont": None, "stats": None}, coff, len(npts), int(poff[-1])


@pytest.fixture(scope="module")
def polygons():
    """about 2,000 polygons of 1 .. 1024 vertices (every family of locscenes.random_polygons, W - 1 = 2047) and the host's
    record of each, computed once"""
    polys = ls.random_polygons(np.random.RandomState(11), 2000)
    assert max(len(p) for p in polys) == 1024 and min(len(p) for p in polys) == 1
    assert max(int(p[:, 0].max()) for p in polys) == 2047 and min(int(p.min()) for p in polys) == 0
    ref = [ls.host_record(p) for p in polys]
    assert sum(bool(np.isnan(r["cx"])) for r in ref) >= 200
    return polys, ref


def into_slots(polys, order, nslots, rs):
    """the polygons, in `order`, dealt into nslots slots of uneven sizes, with an empty and a declined slot in the middle"""
    cuts = np.sort(rs.randint(0, len(order) + 1, nslots - 3))
    groups = [list(g) for g in np.split(np.asarray(order), cuts)]
    mid = len(groups) // 2
    groups[mid:mid] = [[], None]
    return [None if g is None else [polys[k] for k in g] for g in groups], [k for g in groups if g for k in g]


@pytest.mark.parametrize("permuted", [0, 1])
def test_describe_against_the_host_columns(polygons, permuted):
    polys, ref = polygons
    rs = np.random.RandomState(5 + permuted)
    order = rs.permutation(len(polys)) if permuted else np.arange(len(polys))
    slots, flat = into_slots(polys, order, 70, rs)
    assert any(s is None for s in slots) and any(s == [] for s in slots) and max(len(s or []) for s in slots) > 64
    tc, coff, nc, nv = contour_list(slots)
    assert nc == len(polys)
    got = hip.desc_records(hip.describe_contours(tc, cont_cap=nc, pts_cap=nv), nc)
    for j, k in enumerate(flat):
        assert ls.same_bits(got[j], ref[k]), (j, k, got[j], ref[k])
        assert got[j]["npts"] == len(polys[k])


def test_describe_writes_nothing_past_its_capacities(polygons):
    polys, ref = polygons
    slots = [polys[:90], polys[90:100], polys[100:101]]
    tc, coff, nc, nv = contour_list(slots)
    # records: a capacity in the middle of the first slot's second chunk of 64
    raw = hip.describe_contours(tc, cont_cap=nc, pts_cap=nv, desc_cap=70)
    assert raw.shape[0] == 70
    got = hip.desc_records(raw)
    for j in range(70):
        assert ls.same_bits(got[j], ref[j])
    # vertices: a contour whose vertices reach the capacity is left alone, the ones before it are described
    cut = sum(len(p) for p in polys[:50])
    raw = hip.describe_contours(tc, cont_cap=nc, pts_cap=cut)
    got = hip.desc_records(raw)
    for j in range(50):
        assert ls.same_bits(got[j], ref[j])
    assert not raw[50:].any()
    # contours: entries past cont_cap were never written by the tracer
    raw = hip.describe_contours(tc, cont_cap=95, pts_cap=nv, desc_cap=nc)
    got = hip.desc_records(raw)
    for j in range(95):
        assert ls.same_bits(got[j], ref[j])
    assert not raw[95:].any()


# ---- K7b -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    mc, mb = hip.localize_limits()
    slots, stacks, masks, expect = ls.hand_made(mc, mb)
    status, off, desc = ls.pack(slots)
    refs = [ls.ref_localize(s, masks, status, off, desc, len(desc), mc, mb) for s in stacks]
    dmasks = [tuple(None if m is None else torch.from_numpy(m).to(DEV) for m in pair) for pair in masks]
    return stacks, masks, dmasks, status, off, desc, refs, (mc, mb)


def check(res, refs):
    for i, (r, e) in enumerate(zip(res, refs)):
        assert r["status"] == e["status"], (i, r, e)
        if e["status"] != ls.DONE:
            assert (r["nrects"], r["nbubbles"]) == (0, 0)
            continue
        assert r["nrects"] == len(e["rects"]) and r["nbubbles"] == len(e["bubbles"]), (i, r, e)
        assert r["rects"] == e["rects"], (i, r, e)
        assert r["bubbles"] == e["bubbles"], (i, r, e)


def test_localize_hand_made_stacks(hand):
    stacks, masks, dmasks, status, off, desc, refs, _ = hand
    assert len(stacks) == 64
    d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1, 80)).to(DEV)
    for order in (np.arange(len(stacks)), np.random.RandomState(3).permutation(len(stacks))):
        res, tot, _ = hip.localize_stacks([stacks[i] for i in order], dmasks, dev(status), dev(off), d_desc)
        check(res, [refs[i] for i in order])
        done = [refs[i] for i in order if refs[i]["status"] == ls.DONE]
        assert tot == [sum(len(r["rects"]) for r in done), sum(len(r["bubbles"]) + sum(map(len, r["bubbles"])) for r in done)]
        # the parts of the lists do not overlap
        spans = sorted((r["rect_off"], r["nrects"]) for r in res if r["status"] == 0 and r["nrects"])
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))
        spans = sorted((r["track_off"], r["ntrack"]) for r in res if r["status"] == 0 and r["ntrack"])
        assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))


def test_localize_incomplete_records(hand):
    """records beyond ndesc (the contour lists overflowed): exactly the stacks that reach them are declined"""
    stacks, masks, dmasks, status, off, desc, refs, (mc, mb) = hand
    nd = int(off[len(off) // 2])
    d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1, 80)).to(DEV)
    res, _, _ = hip.localize_stacks(stacks, dmasks, dev(status), dev(off), d_desc, ndesc=nd)
    cut = [ls.ref_localize(s, masks, status, off, desc, nd, mc, mb) for s in stacks]
    assert {r["status"] for r in cut} >= {ls.DONE, ls.INCOMPLETE}
    check(res, cut)


def test_localize_lists_one_short(hand):
    """the overflow convention: true totals, nothing written past a capacity, and every stack that got its part is right"""
    stacks, masks, dmasks, status, off, desc, refs, _ = hand
    d_desc = torch.from_numpy(desc.view(np.uint8).reshape(-1, 80)).to(DEV)
    _, tot, _ = hip.localize_stacks(stacks, dmasks, dev(status), dev(off), d_desc)
    for rc, tc in ((tot[0] - 1, tot[1]), (tot[0], tot[1] - 1), (1, 1)):
        res, tot2, (R, T) = hip.localize_stacks(stacks, dmasks, dev(status), dev(off), d_desc, rect_cap=rc, track_cap=tc, guard=64)
        assert tot2 == tot
        assert (R[rc:] == -1).all() and (T[tc:] == -1).all()
        lost_r = lost_t = 0
        for r, e in zip(res, refs):
            assert r["status"] == e["status"] and r["nrects"] == len(e["rects"]) and r["nbubbles"] == len(e["bubbles"])
            if e["status"] != ls.DONE:
                continue
            lost_r += r["rects"] is None
            lost_t += r["bubbles"] is None
            assert r["rects"] in (None, e["rects"]) and r["bubbles"] in (None, e["bubbles"])
        assert (lost_r >= 1) == (rc < tot[0]) and (lost_t >= 1) == (tc < tot[1])


def test_describe_then_localize_random_polygons():
    """K7b behind K7a: 64 stacks of small random polygons in a 200 x 100 frame with both masks, 0 .. 10 tracking slots,
    against the reference localizer on describe()'s records"""
    rs = np.random.RandomState(21)
    W, H = 200, 100
    fid = np.zeros((H, W), np.uint8)
    fid[8:92, 10:190] = 255
    bel = np.zeros((H, W), np.uint8)
    bel[75:92, 30:170] = 255
    masks = [(fid, bel), (fid, None), (None, None)]

    def poly(cx, cy):
        kind = rs.randint(4)
        if kind == 0:
            return np.array([[cx, cy]], np.int32)
        if kind == 1:
            return np.array([[cx, cy], [min(cx + rs.randint(1, 6), W - 1), cy]], np.int32)
        w, h = rs.randint(1, 9), rs.randint(1, 9)
        x1, y1 = min(cx + w, W - 1), min(cy + h, H - 1)
        p = np.array([[cx, cy], [cx, y1], [x1, y1], [x1, cy]], np.int32)
        return p[::-1].copy() if kind == 3 else p

    slots, stacks = [], []
    for s in range(64):
        nb = rs.randint(0, 4)
        centres = [(rs.randint(0, W - 10), rs.randint(0, H - 10)) for _ in range(nb)]
        noise = lambda: [poly(rs.randint(0, W), rs.randint(0, H)) for _ in range(rs.randint(0, 5))]
        g = len(slots)
        slots.append([poly(*c) for c in centres] + noise())
        nt = [0, 10, rs.randint(1, 10)][s % 3]
        tr = []
        for k in range(nt):
            tr.append(len(slots))
            moved = [poly(max(cx - rs.randint(0, 4) * (k + 1), 0), min(max(cy + rs.randint(-2, 3), 0), H - 1)) for cx, cy in centres]
            slots.append(noise() + moved)
        stacks.append({"cam": s % 3, "genesis": g, "track": tr, "bad": 0})
    tc, coff, nc, nv = contour_list(slots)
    status, off, desc = ls.pack([[ls.describe(p) for p in s] for s in slots])
    raw = hip.describe_contours(tc, cont_cap=nc, pts_cap=nv)
    got = hip.desc_records(raw, nc)
    for j in range(nc):
        assert ls.same_bits(got[j], desc[j]), j
    mc, mb = hip.localize_limits()
    refs = [ls.ref_localize(s, masks, status, off, desc, nc, mc, mb) for s in stacks]
    assert sum(len(b) >= 3 for r in refs for b in r["bubbles"]) >= 10 and {r["status"] for r in refs} >= {ls.DONE}
    dmasks = [tuple(None if m is None else torch.from_numpy(m).to(DEV) for m in pair) for pair in masks]
    res, _, _ = hip.localize_stacks(stacks, dmasks, tc["status"], tc["cont_off"], raw, ndesc=nc)
    check(res, refs)
