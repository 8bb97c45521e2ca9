"""K6 (abub_trigger.hip) against the reference model of trigscenes.py, which is AnalyzerUnit::FindTriggerFrame on the host's
significanceFromHist: every field of every result, and the main-loop significances bit for bit.  The histograms are
synthetic, so no frame slab is needed."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import trigscenes as ts  # noqa: E402
from autobub3hs_amd import hip, host  # noqa: E402

W, H = 1280, 96
P = W * H


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def _check(cases, dev, sm, refs=None, what=""):
    refs = [ts.ref_of(c) for c in cases] if refs is None else refs
    for k, (c, d, r) in enumerate(zip(cases, dev, refs)):
        assert ts.same_result(d, r), (what, k, c.get("kind"), len(c["hists"]), c["tss"], d, {f: r[f] for f in ts.FIELDS})
        row = sm[k]
        for i in range(len(c["hists"])):
            if i in r["main"]:
                v = r["main"][i]
                assert row[i] == v or (math.isnan(row[i]) and math.isnan(v)), (what, k, i, row[i], v)
            else:
                assert math.isnan(row[i]), (what, k, i)  # left alone
    return refs


@pytest.fixture(scope="module")
def random_set():
    """256 stacks, their reference results, and the retries behind the first trigger -- computed once"""
    mf, _ = hip.trigger_search_limits()
    counts = [5, 6, 7, 12, 41, 63, 64] + ([65, mf] if mf > 64 else [])
    cases = ts.random_cases(3, 256, counts, P)
    refs = [ts.ref_of(c) for c in cases]
    trig = [k for k, r in enumerate(refs) if r["status"] == 0]
    retries = [dict(cases[k], start=refs[k]["trig"] + 1) for k in trig]
    rrefs = [ts.ref_of(c) for c in retries]
    # not trivia: both outcomes, and retries that find a second trigger
    assert len(trig) >= 40 and len(cases) - len(trig) >= 40
    assert sum(r["status"] == 0 for r in rrefs) >= 10
    assert {len(c["hists"]) for c in cases} == set(counts)
    return cases, refs, retries, rrefs


def test_random_stacks(random_set):
    cases, refs, retries, rrefs = random_set
    dev, sm = ts.run_device(cases, W, H)
    _check(cases, dev, sm, refs, "first")
    dev, sm = ts.run_device(retries, W, H)
    _check(retries, dev, sm, rrefs, "retry")


def test_order_independence(random_set):
    """the same stacks in a permuted order, with other neighbours (a part of the set, retries mixed in)"""
    cases, refs, retries, rrefs = random_set
    rs = np.random.RandomState(5)
    mixed = cases[::2] + retries
    mrefs = refs[::2] + rrefs
    order = rs.permutation(len(mixed))
    dev, sm = ts.run_device(mixed, W, H, order)
    _check(mixed, dev, sm, mrefs, "permuted")


def test_arithmetic_edges():
    cases = ts.edge_cases()
    nan = inf = 0
    refs = []
    for c in cases:
        tr = []
        refs.append(ts.ref_of(c, None, tr))
        nan += sum(math.isnan(v) for _, _, _, v in tr)
        inf += sum(math.isinf(v) for _, _, _, v in tr)
    assert nan >= 20 and inf >= 5
    dev, sm = ts.run_device(cases, 512, 512)
    _check(cases, dev, sm, refs, "edges")
    # retries behind the triggers of the constant-column stacks: the +-inf frames are history now
    retries = [dict(c, start=r["trig"] + 1) for c, r in zip(cases, refs) if r["status"] == 0]
    assert len(retries) >= 5
    dev, sm = ts.run_device(retries, 512, 512)
    _check(retries, dev, sm, None, "edge retries")


def _lazy_cases():
    F = 41

    def case(t0, cov=None, pend=None, flicker=None, seed=1):
        c = dict(hists=ts.step_stack(seed + t0, F, t0, P, flicker), P=P, tss=10, start=1, first_bad=F)
        c["covered"] = np.ones(F, bool)
        c["pending"] = np.zeros(F, bool)
        if cov is not None:
            c["covered"][:] = False
            for a, b in cov:
                c["covered"][a:b] = True
        for i in pend or ():
            c["pending"][i] = True
        return c

    cases = [case(30, cov=[(1, 24)]), case(22, cov=[(1, 24)]), case(10, pend=[20], seed=7), case(12, pend=[9]), case(12, pend=[14]),
             case(12, pend=[13]), case(30, cov=[(1, 10), (15, 41)]), case(8, cov=[(1, 11), (15, 41)], seed=2),
             case(20, cov=[(1, 12)], flicker=9)]
    want = [(ts.NEED_FRAMES, 24), (ts.NEED_FRAMES, 24), (ts.DONE, 0), (ts.NEED_FINAL, 9), (ts.NEED_FINAL, 14),
            (ts.NEED_FINAL, 13), (ts.NEED_FRAMES, 10), (ts.DONE, 0), (ts.NEED_FRAMES, 12)]
    return cases, want


def test_laziness():
    cases, want = _lazy_cases()
    full = [ts.ref_of(dict(c, covered=None, pending=None)) for c in cases]
    for c, f, t0 in zip(cases, full, (30, 22, 10, 12, 12, 12, 30, 8, 20)):
        assert (f["state"], f["status"], f["trig"]) == (ts.DONE, 0, t0)  # the scenes trigger where they were built to
    dev, sm = ts.run_device(cases, W, H)
    refs = _check(cases, dev, sm, None, "lazy")
    assert [(r["state"], r["need_frame"]) for r in refs] == want
    # coverage granted in instalments (five more frames, or the one pending frame made final) until every search is done
    cur = [dict(c, covered=c["covered"].copy(), pending=c["pending"].copy()) for c in cases]
    for _ in range(64):
        dev, sm = ts.run_device(cur, W, H)
        _check(cur, dev, sm, None, "instalment")
        if all(d["state"] == ts.DONE for d in dev):
            break
        for c, d in zip(cur, dev):
            if d["state"] == ts.NEED_FRAMES:
                assert not c["covered"][d["need_frame"]]
                c["covered"][d["need_frame"]:d["need_frame"] + 5] = True
            elif d["state"] == ts.NEED_FINAL:
                assert c["pending"][d["need_frame"]]
                c["pending"][d["need_frame"]] = False
    else:
        raise AssertionError("the instalments never ended")
    for d, f in zip(dev, full):
        assert ts.same_result(d, f), (d, f)


def test_first_bad_and_short_stacks():
    F = 41
    quiet = ts.step_stack(20, F, 40, P)
    quiet[40] = quiet[39]
    trig = ts.step_stack(4, F, 20, P)
    cases = [dict(hists=quiet, P=P, tss=10, first_bad=7), dict(hists=quiet, P=P, tss=10, first_bad=1),
             dict(hists=trig, P=P, tss=10, first_bad=21), dict(hists=trig, P=P, tss=10, first_bad=22),
             dict(hists=trig, P=P, tss=10, first_bad=20), dict(hists=trig, P=P, tss=10, first_bad=23),
             dict(hists=trig, P=P, tss=2, first_bad=21, start=5), dict(hists=trig[:4], P=P, tss=10),
             dict(hists=trig[:4], P=P, tss=10, first_bad=0), dict(hists=trig[:5], P=P, tss=10),
             # an undecodable frame that no segment covers either, and one behind a missing frame
             dict(hists=quiet, P=P, tss=10, first_bad=7, covered=np.arange(F) < 7),
             dict(hists=quiet, P=P, tss=10, first_bad=9, covered=np.arange(F) < 7)]
    dev, sm = ts.run_device(cases, W, H)
    refs = _check(cases, dev, sm, None, "first_bad")
    got = [(r["state"], r["status"]) for r in refs]
    assert got[0] == (ts.DONE, -9) and refs[0]["loc_thres"] >= 2 and refs[0]["evaluated"] == 6
    assert got[1] == (ts.DONE, -9) and refs[1]["loc_thres"] == -1
    assert got[2][0] == ts.BAD_LOOKAHEAD and got[3][0] == ts.BAD_LOOKAHEAD
    assert got[4] == (ts.DONE, -9) and got[5] == (ts.DONE, 0)
    assert got[7] == (ts.DONE, -9) and got[8] == (ts.DONE, -9)
    assert got[10] == (ts.DONE, -9) and (refs[11]["state"], refs[11]["need_frame"]) == (ts.NEED_FRAMES, 7)


def test_clear_pending():
    """abub_trigger_clear_pending_dev: pending[j] = 0 exactly where done[j] != 0, at a size that is no multiple of the block"""
    from autobub3hs_amd import _lib
    rs = np.random.RandomState(2)
    n = 3 * 256 + 77
    p, d = rs.randint(0, 2, n + 64).astype(np.uint8), rs.randint(0, 3, n + 64).astype(np.uint8)
    tp, td = torch.from_numpy(p).cuda(), torch.from_numpy(d).cuda()
    _lib.check(_lib.lib().abub_trigger_clear_pending_dev(tp.data_ptr(), td.data_ptr(), n, torch.cuda.current_stream().cuda_stream))
    want = p.copy()
    want[:n][d[:n] != 0] = 0  # nothing behind n is touched
    assert np.array_equal(tp.cpu().numpy(), want)
