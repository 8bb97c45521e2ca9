"""Per-frame statistics on the GPU: abub_frame_stats_dev against the numpy restatement (tests/surveyref.py), bit for bit, at
every size at which it takes another path (the seams of unit, wave, tile and grid), with the three streams at every residue
mod 16 and in all three load widths, on the contents of tests/test_survey_abi.py; what a launch is made of (many jobs, any
order, a reused results buffer); the grid's loop; sums past 2^32; the range status; canaries; the argument refusals."""

import numpy as np
import pytest
import torch

import surveyref
from autobub3hs_amd import _lib, hip, host
from test_survey_abi import SIZES, stat_contents

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GARBAGE = 0x5A
NONE = hip.STAT_NONE
E_INVALID = -1
# (cur, ref, model) mod 16: every residue of every stream, in each load width: all congruent mod 16 (16-byte loads),
# congruent mod 4 only (4-byte loads), not congruent (single bytes)
RESIDUES = [(r, r, r) for r in range(16)] + [(r, (r + 4) % 16, (r + 8) % 16) for r in range(16)] + \
           [(r, (r + 1) % 16, (r + 2) % 16) for r in range(16)]


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


class Layout:
    """frames and models laid into two buffers of other bytes at chosen residues mod 16, with gaps between them"""

    def __init__(self):
        self.frames, self.models, self.f_at, self.m_at = [], [], 16, 16

    def _place(self, pieces, at, data, size, mod):
        at = ((at + 15) & ~15) + 16 + mod
        pieces.append((at, data))
        return at, at + size

    def frame(self, data, mod):
        off, self.f_at = self._place(self.frames, self.f_at, data, len(data), mod)
        return off

    def model(self, mu, s6, mod):
        off, self.m_at = self._place(self.models, self.m_at, (mu, s6), len(mu), mod)
        return off

    def tensors(self):
        fb = (np.arange(self.f_at + 48, dtype=np.uint32) * 37 >> 3).astype(np.uint8)
        mb = (np.arange(self.m_at + 48, dtype=np.uint32) * 29 >> 2).astype(np.uint8)
        sb = (np.arange(self.m_at + 48, dtype=np.uint32) * 13 >> 1).astype(np.uint8)
        for at, d in self.frames:
            fb[at:at + len(d)] = d
        for at, (mu, s6) in self.models:
            mb[at:at + len(mu)] = mu
            sb[at:at + len(s6)] = s6
        t = [torch.from_numpy(b).to(DEV) for b in (fb, mb, sb)]
        assert all(x.data_ptr() % 16 == 0 for x in t)
        return fb, t


def launch(frames, jobs, n, mu=None, s6=None, **kw):
    """one call with the results between canaries and full of garbage -> the records; the canaries must be whole"""
    m = len(jobs)
    full = torch.full((64 + 64 * m + 64,), GARBAGE, dtype=torch.uint8, device=DEV)
    got = hip.frame_stats(frames, jobs, n, mu, s6, results=full[64:64 + 64 * m], **kw)
    whole = full.cpu().numpy()
    assert (whole[:64] == GARBAGE).all() and (whole[64 + 64 * m:] == GARBAGE).all(), "a canary was written"
    return got


def jobs_of(n, rs, residues=RESIDUES):
    """every content of stat_contents at every combination of residues -> (layout, job rows, wanted rows)"""
    lay, jobs, want = Layout(), [], []
    for k, (cur, ref, mu, s6) in enumerate(stat_contents(n, rs)):
        rec = surveyref.kernel_row(surveyref.record(cur, ref if mu is not None else None, mu, s6))
        for rc, rr, rm in residues:
            c = lay.frame(cur, rc)
            r = c if ref is cur else NONE if ref is None else lay.frame(ref, rr)
            jobs.append((c, r, NONE if mu is None else lay.model(mu, s6, rm)))
            want.append(rec)
    return lay, jobs, np.array(want, dtype=np.uint64)


@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_numpy(n):
    rs = np.random.RandomState(n % 9973)
    lay, jobs, want = jobs_of(n, rs)
    host_frames, (F, M, S) = lay.tensors()
    widths = {(0 if (c ^ r) % 16 == 0 and (c ^ m) % 16 == 0 else 1 if (c ^ r) % 4 == 0 and (c ^ m) % 4 == 0 else 2)
              for c, r, m in jobs if r != NONE and m != NONE and r != c}
    assert widths == {0, 1, 2} and {c % 16 for c, _, _ in jobs} == set(range(16))
    assert {r % 16 for _, r, _ in jobs if r != NONE} == {m % 16 for _, _, m in jobs if m != NONE} == set(range(16))
    got = launch(F, jobs, n, M, S)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (n, bad[:5], [jobs[i] for i in bad[:5]], got[bad[:5]], want[bad[:5]])
    assert np.array_equal(F.cpu().numpy(), host_frames), "the frames were written"
    # mu == NULL: no job has a model, whatever its model offset says; a reference frame alone gives no column
    bare = np.array([surveyref.kernel_row(surveyref.record(host_frames[c:c + n])) for c, _, _ in jobs[::7]], dtype=np.uint64)
    assert np.array_equal(launch(F, jobs[::7], n), bare)


def test_a_launch_is_the_sum_of_its_jobs_in_any_order():
    n = 4099
    rs = np.random.RandomState(5)
    lay, jobs, want = jobs_of(n, rs, residues=RESIDUES[::8])
    _, (F, M, S) = lay.tensors()
    got = launch(F, jobs, n, M, S)
    assert np.array_equal(got, want)
    order = rs.permutation(len(jobs))
    assert np.array_equal(launch(F, [jobs[i] for i in order], n, M, S), want[order])
    one_by_one = np.concatenate([launch(F, [jobs[i]], n, M, S) for i in order])
    assert np.array_equal(one_by_one, want[order])
    # a reused results buffer: what the launch before left there does not show
    res = torch.full((64 * len(jobs),), GARBAGE, dtype=torch.uint8, device=DEV)
    first = hip.frame_stats(F, jobs, n, M, S, results=res)
    again = hip.frame_stats(F, jobs[::-1], n, M, S, results=res)
    assert np.array_equal(first, want) and np.array_equal(again, want[::-1])


def test_seventy_thousand_jobs_of_one_byte():
    """more jobs than the grid's y takes: it loops"""
    m = 70000
    rs = np.random.RandomState(7)
    p, mu, s6 = (rs.randint(0, 256, m).astype(np.uint8) for _ in range(3))
    s6[::3] = 0
    F, M, S = (torch.from_numpy(a).to(DEV) for a in (p, mu, s6))
    ref = np.maximum(np.arange(m) - 2, 0)
    jobs = np.stack([np.arange(m), ref, np.arange(m)], axis=1)
    pi, out = p.astype(np.int64), np.maximum(np.abs(p.astype(np.int64) - mu) - s6, 0)
    moved = np.maximum(np.abs(pi - pi[ref]) - s6, 0)
    want = np.stack([0 * pi, pi, pi, pi == 0, pi == 255, out > 0, moved > 0, 3 + 0 * pi, pi, pi * pi, out, moved], axis=1).astype(np.uint64)
    assert want[:, 5].sum() > 1000 and want[:, 6].sum() > 1000
    assert np.array_equal(launch(F, jobs.tolist(), 1, M, S), want)


def test_sums_past_2_to_the_32():
    n = 1680 * 1050
    F = torch.full((n,), 255, dtype=torch.uint8, device=DEV)
    Z = torch.zeros((n,), dtype=torch.uint8, device=DEV)
    got = launch(F, [(0, NONE, NONE), (0, 0, 0)], n, Z, Z)
    raw = [255, 255, 0, n, 0, 0]
    assert n * 255 * 255 > 1 << 32
    assert list(got[0]) == [0] + raw + [0, n * 255, n * 255 * 255, 0, 0]
    assert list(got[1]) == [0, 255, 255, 0, n, n, 0, 3, n * 255, n * 255 * 255, n * 255, 0]


def test_range_status():
    """the offsets stay inside the real tensors, or the job is one the kernel must not read: only the sizes it is told are small"""
    n, nf = 1000, 10
    rs = np.random.RandomState(11)
    fr = rs.randint(0, 256, (nf, n)).astype(np.uint8)
    mu, s6 = rs.randint(0, 256, (nf, n)).astype(np.uint8), rs.randint(0, 40, (nf, n)).astype(np.uint8)
    F, M, S = (torch.from_numpy(a.reshape(-1)).to(DEV) for a in (fr, mu, s6))
    jobs = [(i * n, max(i - 2, 0) * n, i * n) for i in range(nf)]
    want = np.array([surveyref.kernel_row(surveyref.record(fr[i], fr[max(i - 2, 0)], mu[i], s6[i])) for i in range(nf)], dtype=np.uint64)
    assert np.array_equal(launch(F, jobs, n, M, S), want)
    for kw, out in ((dict(frames_bytes=7 * n - 1), [6, 7, 8, 9]),            # cur one byte past
                    (dict(model_bytes=3 * n + 999), [3, 4, 5, 6, 7, 8, 9]),  # the model one byte past
                    (dict(frames_bytes=10 * n, model_bytes=10 * n - 1), [9]), (dict(frames_bytes=n - 1), list(range(nf))),
                    (dict(frames_bytes=10 * n, model_bytes=10 * n), [])):
        got = launch(F, jobs[::-1], n, M, S, **kw)[::-1]
        for i in range(nf):
            assert np.array_equal(got[i], surveyref.RANGE_ROW if i in out else want[i]), (kw, i, got[i])
    # the reference frame alone one byte past (jobs in reverse: frame i against frame i + 2), with and without a model
    back = [(i * n, min(i + 2, nf - 1) * n, i * n) for i in range(nf)]
    wantb = np.array([surveyref.kernel_row(surveyref.record(fr[i], fr[min(i + 2, nf - 1)], mu[i], s6[i])) for i in range(nf)], dtype=np.uint64)
    got = launch(F, back, n, M, S, frames_bytes=9 * n + n - 1)
    for i in range(nf):
        assert np.array_equal(got[i], surveyref.RANGE_ROW if i >= 7 else wantb[i]), (i, got[i])
    got = launch(F, back, n, frames_bytes=9 * n + n - 1)
    assert [int(g[0]) for g in got] == [0] * 7 + [1] * 3 and all(not g[1:].any() for g in got[7:])
    # offsets near 2^64, each stream in turn, between two good jobs
    top = (1 << 64) - 2
    for bad in ((top, NONE, NONE), (top - n, 0, 0), (0, top, 0), (0, top - n + 1, NONE), (0, 0, top), (n, NONE, top - n + 1),
                ((1 << 64) - 1, NONE, NONE)):
        got = launch(F, [jobs[3], bad, jobs[5]], n, M, S)
        assert np.array_equal(got[0], want[3]) and np.array_equal(got[2], want[5]) and list(got[1]) == surveyref.RANGE_ROW, (bad, got)


def test_nothing_to_do_and_the_argument_refusals():
    L = _lib.lib()
    buf = torch.full((4096,), GARBAGE, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    assert p % 16 == 0
    assert hip.frame_stats(buf, [], 64, buf, buf, results=buf[1024:]).shape == (0, 12)
    ok = dict(frames=p, frames_bytes=4096, mu=p, sigma6=p, model_bytes=4096, jobs=p, njobs=1, frame_bytes=64, results=p + 2048, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_frame_stats_dev(a["frames"], a["frames_bytes"], a["mu"], a["sigma6"], a["model_bytes"], a["jobs"], a["njobs"],
                                      a["frame_bytes"], a["results"], a["stream"])

    for kw in (dict(frames=None), dict(jobs=None), dict(results=None), dict(sigma6=None), dict(njobs=-1), dict(frame_bytes=0),
               dict(frame_bytes=(1 << 32) - 1), dict(jobs=p + 4), dict(results=p + 2052)):
        assert call(**kw) == E_INVALID, kw
        assert b"abub_frame_stats_dev" in L.abub_last_error(), kw
    assert call(njobs=0) == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == GARBAGE).all(), "a refused or empty call wrote something"
