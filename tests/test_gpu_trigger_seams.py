"""K6 (abub_trigger.hip) on the designed scenes of trigscenes.py: decisions at the seams of its 64-frame tiles, counts beyond
the first 64-bin chunk, NaN / inf histories carried over a seam, and P above 2^24 where the reference's float pixel counter
rounds.  Every field of every result and every main-loop significance is compared bit for bit with the reference model on
the host's significanceFromHist, as test_gpu_trigger.py does; tests/test_trigger_abi.py holds (on the CPU) that the scenes
reach what they were built for.  The histograms are synthetic, so no frame slab is needed."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import trigscenes as ts  # noqa: E402
from autobub3hs_amd import hip, host  # noqa: E402
from test_gpu_trigger import _check  # noqa: E402

W, H = 1280, 96


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def _with_retries(cases):
    """-> (cases, their references, the retries behind every trigger, their references)"""
    refs = [ts.ref_of(c) for c in cases]
    retries = [dict(c, start=r["trig"] + 1) for c, r in zip(cases, refs) if r["state"] == ts.DONE and r["status"] == 0]
    return cases, refs, retries, [ts.ref_of(c) for c in retries]


@pytest.fixture(scope="module")
def limit():
    return hip.trigger_search_limits()[0]


@pytest.fixture(scope="module")
def seam_set(limit):
    return _with_retries(ts.seam_cases(limit=limit))


@pytest.fixture(scope="module")
def chunk_set(limit):
    return _with_retries(ts.chunk_cases(limit=limit))


def _two_launches(s, w, h, what):
    cases, refs, retries, rrefs = s
    assert len(retries) >= 1
    dev, sm = ts.run_device(cases, w, h)
    _check(cases, dev, sm, refs, what)
    dev, sm = ts.run_device(retries, w, h)
    _check(retries, dev, sm, rrefs, what + " retries")


def test_seam_scenes(seam_set):
    """steps, flickers, retries, first_bad, the end of the coverage and pending frames at s - 2 .. s + 2 of a tile seam"""
    _two_launches(seam_set, W, H, "seams")


def test_chunk_scenes(chunk_set):
    """counts up to bin 255 in stacks of two and three tiles (and one at the frame limit)"""
    _two_launches(chunk_set, W, H, "chunks")


def test_arithmetic_edges_across_a_seam():
    """wrapped squares, constant columns and frames that stop below earlier ones, with the changes at s - 1 .. s + 2"""
    _two_launches(_with_retries([c for F in (70, 131) for c in ts.edge_cases(F=F)]), 512, 512, "seam edges")


def test_large_p():
    """P above 2^24, up to the largest the entry takes: the float pixel counter ends short or over, counts are pushed
    rounded; each (W, H) is a launch of its own"""
    cases, refs, retries, rrefs = _with_retries(ts.large_p_cases())
    assert len(retries) >= len(ts.LARGE_P)
    for w, h in ts.LARGE_P:
        for cs, rs, what in ((cases, refs, "large P"), (retries, rrefs, "large P retries")):
            pick = [k for k, c in enumerate(cs) if (c["W"], c["H"]) == (w, h)]
            assert pick
            dev, sm = ts.run_device([cs[k] for k in pick], w, h)
            _check([cs[k] for k in pick], dev, sm, [rs[k] for k in pick], "%s %d x %d" % (what, w, h))


def test_a_stack_does_not_depend_on_its_neighbours(limit):
    """the seam and chunk scenes in a permuted order, interleaved with 32 twelve-frame stacks of edge_cases(): the prefix
    sums and the previous tile's last frame that a block keeps in LDS are set up per pass for the block's one stack, and
    what its neighbours in the launch are changes nothing"""
    P = 512 * 512
    big = ts.seam_cases(P, limit) + ts.chunk_cases(P, limit)
    small = ts.edge_cases(P)
    small = (small + small)[:32]
    rs = np.random.RandomState(17)
    big = [big[k] for k in rs.permutation(len(big))]
    step = len(big) // len(small)
    mixed = []
    for k, c in enumerate(big):
        mixed.append(c)
        if k % step == step - 1 and k // step < len(small):
            mixed.append(small[k // step])
    assert len(mixed) == len(big) + len(small)
    refs = [ts.ref_of(c) for c in mixed]
    dev, sm = ts.run_device(mixed, 512, 512)
    _check(mixed, dev, sm, refs, "interleaved")
    dev, sm = ts.run_device(mixed, 512, 512, rs.permutation(len(mixed)))
    _check(mixed, dev, sm, refs, "interleaved, permuted")


def test_instalments_across_a_seam(seam_set):
    """the stacks covered up to s - 1: one more frame per round until every search is done, every round against the
    reference; the last answer is that of the fully covered stack"""
    cases = [c for c in seam_set[0] if c["what"] == "covered" and c["end"] == c["seam"] - 1]
    assert len(cases) >= 2 * len(ts.seam_sets())
    full = [ts.ref_of(dict(c, covered=None, pending=None)) for c in cases]
    for c, f in zip(cases, full):  # (a step in the last two frames has no second look-ahead: 67 frames, and 131 at s = 128)
        assert (f["status"] == 0 and f["trig"] == c["t0"]) == (c["t0"] + 2 < len(c["hists"])), (c["t0"], f)
    cur = [dict(c, covered=c["covered"].copy()) for c in cases]
    for rounds in range(1, 17):
        dev, sm = ts.run_device(cur, W, H)
        _check(cur, dev, sm, None, "instalment %d" % rounds)
        if all(d["state"] == ts.DONE for d in dev):
            break
        for c, d in zip(cur, dev):
            if d["state"] != ts.DONE:
                assert d["state"] == ts.NEED_FRAMES and not c["covered"][d["need_frame"]]
                c["covered"][d["need_frame"]] = True
    else:
        raise AssertionError("the instalments never ended")
    assert rounds >= 4  # s, s + 1, s + 2 were each asked for
    for d, f in zip(dev, full):
        assert ts.same_result(d, f), (d, f)
