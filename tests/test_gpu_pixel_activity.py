"""Per-pixel activity planes on the GPU: abub_pixel_activity_dev against the numpy restatement (tests/activityref.py), bit for
bit: at every frame size at which it takes another path (a thread's run of 8 pixels, its block of 256 threads = 2048 pixels,
the head and tail bytes), on the contents of tests/test_survey_abi.py with and without a model, with the four streams at
residues mod 16 that reach each load width (8, 4, 1 bytes) with each stream as the odd one out, on planes that start at
random values between canaries; job lists of every form in one call, in two calls and permuted; the range status; the
identity with abub_frame_stats_dev's records; one full-size case; the argument refusals."""
import numpy as np
import pytest
import torch

import activityref
from autobub3hs_amd import _lib, hip, host
from test_survey_abi import stat_contents

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NONE = hip.STAT_NONE
E_INVALID = -1
PX, BLOCK = hip.ACT_PIXELS_PER_THREAD, 256 * hip.ACT_PIXELS_PER_THREAD  # a thread's run of pixels; a block's
assert (PX, BLOCK) == (8, 2048)
SIZES = [1, 3, 15, 16, 17, 64, 255, 960, 1023, 1025, 16383, 16384, 16401, PX - 1, PX, PX + 1, BLOCK - 1, BLOCK, BLOCK + 1]
CANARY = 0xC0FFEE11
GUARD = 64  # words in front of and behind the planes
# (cur, ref, mu, sigma6) mod 16.  All congruent mod 16 (8-byte loads after the head bytes); congruent mod 4 only; each stream
# in turn the odd one out by 8 (still 8-byte loads), by 4 (that stream in 4-byte loads) and by 1 (in bytes); none congruent
RESIDUES = [(r, r, r, r) for r in range(16)] + [(r, (r + 4) % 16, (r + 8) % 16, (r + 12) % 16) for r in range(16)] + \
           [tuple((3 * s + d + (d if k == s else 0)) % 16 for k in range(4)) for s in range(4) for d in (8, 4, 1)] + \
           [(r, (r + 1) % 16, (r + 2) % 16, (r + 3) % 16) for r in (0, 5, 10, 15)]
assert len(RESIDUES) == 48


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


class Pool:
    """frames laid into one buffer of other bytes at chosen residues mod 16, with gaps between them"""

    def __init__(self):
        self.pieces, self.at = [], 16

    def frame(self, data, mod=0):
        at = ((self.at + 15) & ~15) + 16 + mod
        self.pieces.append((at, np.asarray(data, np.uint8).reshape(-1)))
        self.at = at + len(self.pieces[-1][1])
        return at

    def tensor(self):
        buf = (np.arange(self.at + 48, dtype=np.uint32) * 37 >> 3).astype(np.uint8)
        for at, d in self.pieces:
            buf[at:at + len(d)] = d
        t = torch.from_numpy(buf).to(DEV)
        assert t.data_ptr() % 16 == 0
        return buf, t


def model_tensors(mu, s6, rm=0, rs=0):
    """mu and sigma6 on the device at addresses with the residues rm and rs mod 16 (None: no model)"""
    if mu is None:
        return None, None
    out = []
    for a, r in ((mu, rm), (s6, rs)):
        t = torch.full((len(a) + 32,), 0x77, dtype=torch.uint8, device=DEV)
        assert t.data_ptr() % 16 == 0
        t[r:r + len(a)] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        out.append(t[r:r + len(a)])
    return out


def expected(buf, jobs, n, mu, s6, start, frames_bytes=None):
    """start + what every job that lies inside the buffer adds, and the status"""
    fb = len(buf) if frames_bytes is None else frames_bytes
    want, status = start.astype(np.int64).copy(), 0
    inside = lambda off: off <= fb and fb - off >= n  # noqa: E731
    for cur, ref in jobs:
        ref = None if ref == NONE or ref < 0 else ref
        if not inside(cur) or (ref is not None and not inside(ref)):
            status = activityref.E_RANGE
            continue
        t = activityref.terms(buf[cur:cur + n], None if ref is None or mu is None else buf[ref:ref + n], mu, s6)
        want[:6 if mu is not None else 2] += t[:6 if mu is not None else 2]
    return want, status


def launch(F, jobs, n, M=None, S=None, start=None, stride=None, rs=None, frames_bytes=None):
    """one call onto planes of random values between canaries -> (the planes [6, n] as int64, the status, the start values);
    the canaries, and the words between the planes where plane_stride > n, must be whole"""
    stride = (n + 3) & ~3 if stride is None else stride
    if start is None:
        start = (rs or np.random.RandomState(n)).randint(0, 1 << 31, (6, n)).astype(np.uint32)
    whole = np.full(GUARD + 6 * stride + GUARD, CANARY, np.uint32)
    body = whole[GUARD:GUARD + 6 * stride].reshape(6, stride)
    body[:, :n] = start
    t = torch.from_numpy(whole.view(np.int32)).to(DEV)
    assert t.data_ptr() % 16 == 0
    status = hip.pixel_activity(F, jobs, n, t[GUARD:], M, S, plane_stride=stride, frames_bytes=frames_bytes)
    after = t.cpu().numpy().view(np.uint32)
    got = after[GUARD:GUARD + 6 * stride].reshape(6, stride)
    assert (after[:GUARD] == CANARY).all() and (after[GUARD + 6 * stride:] == CANARY).all(), "a canary was written"
    assert (got[:, n:] == CANARY).all(), "a word between the planes was written"
    return got[:, :n].astype(np.int64), status, start


def check(F, buf, jobs, n, mu=None, s6=None, M=None, S=None, **kw):
    got, status, start = launch(F, jobs, n, M, S, **kw)
    want, wstatus = expected(buf, jobs, n, mu, s6, start, kw.get("frames_bytes"))
    assert status == wstatus, (status, wstatus)
    bad = np.argwhere(got != (want & 0xFFFFFFFF))
    assert bad.size == 0, (n, len(jobs), bad[:5], [(got[k, i], want[k, i]) for k, i in bad[:5]])
    if mu is None:
        assert np.array_equal(got[2:], start[2:]), "planes 2 to 5 were touched without a model"
    return got


@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_numpy(n):
    """every content, each at another combination of residues; with the model and without; plane_stride tight and larger"""
    rs = np.random.RandomState(n % 9973)
    for k, (cur, ref, mu, s6) in enumerate(stat_contents(n, rs)):
        rc, rr, rm, rsg = RESIDUES[(7 * k + n) % 48]
        pool = Pool()
        c = pool.frame(cur, rc)
        r = c if ref is cur else NONE if ref is None else pool.frame(ref, rr)
        other = pool.frame(rs.randint(0, 256, n), rr)
        jobs = [(c, r), (other, c), (c, NONE), (other, other)]
        buf, F = pool.tensor()
        M, S = model_tensors(mu, s6, rm, rsg)
        check(F, buf, jobs, n, mu, s6, M, S, rs=rs, stride=((n + 3) & ~3) + (0 if k % 2 else 4 * (1 + k)))
        if mu is not None:
            check(F, buf, jobs, n, rs=rs)  # mu == NULL: planes 2 to 5 are not touched, whatever the jobs' ref says
        assert np.array_equal(F.cpu().numpy(), buf), "the frames were written"


@pytest.mark.parametrize("n", [17, 1025])
def test_every_load_width_with_each_stream_the_odd_one_out(n):
    rs = np.random.RandomState(n)
    frames = rs.randint(0, 256, (3, n)).astype(np.uint8)
    mu, s6 = rs.randint(0, 256, n).astype(np.uint8), rs.randint(0, 40, n).astype(np.uint8)
    for rc, rr, rm, rsg in RESIDUES:
        pool = Pool()
        a, b, c = pool.frame(frames[0], rc), pool.frame(frames[1], rr), pool.frame(frames[2], rc)
        buf, F = pool.tensor()
        M, S = model_tensors(mu, s6, rm, rsg)
        check(F, buf, [(a, b), (c, b), (a, a), (b, a)], n, mu, s6, M, S, rs=rs)


FORMS = ("chain2", "chain1", "noref", "someref", "shuffled", "same", "self")


def job_list(form, length, offs, rs):
    idx = np.arange(length)
    if form == "chain2":
        return [(offs[i], offs[max(i - 2, 0)]) for i in idx]
    if form == "chain1":
        return [(offs[i], offs[max(i - 1, 0)]) for i in idx]
    if form == "noref":
        return [(offs[i], NONE) for i in idx]
    if form == "someref":
        return [(offs[i], NONE if i % 3 == 1 else offs[max(i - 2, 0)]) for i in idx]
    if form == "shuffled":
        return [(offs[i], offs[max(i - 2, 0)]) for i in rs.permutation(length)]
    if form == "same":
        return [(offs[0], offs[min(1, len(offs) - 1)])] * length
    return [(offs[i], offs[i]) for i in idx]


@pytest.mark.parametrize("form", FORMS)
def test_job_lists_in_one_call_in_two_and_permuted(form):
    n = 1025
    rs = np.random.RandomState(len(form))
    nf = 41
    frames = rs.randint(0, 256, (nf, n)).astype(np.uint8)
    frames[5:9] = frames[4]  # (frames that do not move)
    mu, s6 = rs.randint(0, 256, n).astype(np.uint8), rs.randint(0, 30, n).astype(np.uint8)
    pool = Pool()
    offs = [pool.frame(f) for f in frames]
    buf, F = pool.tensor()
    M, S = model_tensors(mu, s6)
    for length in (0, 1, 2, 3, 5, 64, 65, 300):
        jobs = job_list(form, length, [offs[i % nf] for i in range(max(length, 2))], rs)
        start = rs.randint(0, 1 << 31, (6, n)).astype(np.uint32)
        one = check(F, buf, jobs, n, mu, s6, M, S, start=start)
        if length == 0:
            assert np.array_equal(one, start)
            continue
        cut = length // 3
        first, _, _ = launch(F, jobs[:cut], n, M, S, start=start)
        two, _, _ = launch(F, jobs[cut:], n, M, S, start=first.astype(np.uint32))
        assert np.array_equal(two, one), (form, length)
        order = rs.permutation(length)
        perm, _, _ = launch(F, [jobs[i] for i in order], n, M, S, start=start)
        assert np.array_equal(perm, one), (form, length)


def test_range_status():
    """a refusal the kernel makes cleanly: every offset it reads stays inside the real tensor, only the size it is told is
    small, or the job is one it must not read"""
    n, nf = 1000, 10
    rs = np.random.RandomState(11)
    fr = rs.randint(0, 256, (nf, n)).astype(np.uint8)
    mu, s6 = rs.randint(0, 256, n).astype(np.uint8), rs.randint(0, 40, n).astype(np.uint8)
    buf = fr.reshape(-1)
    F = torch.from_numpy(buf).to(DEV)
    M, S = model_tensors(mu, s6)
    jobs = [(i * n, max(i - 2, 0) * n) for i in range(nf)]
    back = [(i * n, min(i + 2, nf - 1) * n) for i in range(nf)]
    for js, fb, status in ((jobs, None, 0), (jobs, 7 * n - 1, 1), (jobs, n - 1, 1), (back, 9 * n + n - 1, 1), (back, 10 * n, 0)):
        for with_model in (True, False):
            args = (mu, s6, M, S) if with_model else ()
            got, st, start = launch(F, js, n, *args[2:], frames_bytes=fb)
            want, wst = expected(buf, js, n, *(args[:2] or (None, None)), start, fb)
            assert st == wst == status and np.array_equal(got, want & 0xFFFFFFFF), (fb, with_model)
    # one job with cur past the end and one with ref past the end among good jobs; offsets near 2^64 must not wrap
    top = (1 << 64) - 2
    for bad_cur, bad_ref in (((10 * n - 999, 0), (0, 10 * n - 999)), ((top, NONE), (0, top)), ((top - n, 0), (n, top - n + 1)),
                             (((1 << 64) - n + 5, NONE), (0, (1 << 64) - n + 5))):  # (off + n wraps to 5)
        js = [jobs[3], bad_cur, jobs[5], bad_ref, jobs[7]]
        got, st, start = launch(F, js, n, M, S)
        want, _ = expected(buf, [jobs[3], jobs[5], jobs[7]], n, mu, s6, start)
        assert st == activityref.E_RANGE and np.array_equal(got, want), (bad_cur, bad_ref)
    # and the status is cleared by the call: a good call after a refused one
    assert launch(F, jobs, n, M, S)[1] == 0


def test_plane_totals_equal_the_frame_records():
    n, nf = 4099, 12
    rs = np.random.RandomState(3)
    fr = rs.randint(0, 256, (nf, n)).astype(np.uint8)
    fr[3, :100], fr[4, 50:200] = 0, 255
    mu, s6 = rs.randint(0, 256, n).astype(np.uint8), rs.randint(0, 60, n).astype(np.uint8)
    F = torch.from_numpy(fr.reshape(-1)).to(DEV)
    M, S = model_tensors(mu, s6)
    jobs = [(i * n, NONE if i == 5 else max(i - 2, 0) * n) for i in range(nf)]
    got, st, _ = launch(F, jobs, n, M, S, start=np.zeros((6, n), np.uint32))
    rec = hip.frame_stats(F, [(c, r, 0) for c, r in jobs], n, M, S)
    cols = {name: k for k, name in enumerate(hip.STAT_COLUMNS)}
    assert st == 0 and not rec[:, 0].any()
    assert [int(v) for v in got.sum(axis=1)] == [int(rec[:, cols[name]].sum()) for name in activityref.PLANES]


def test_full_size_chain_with_a_model():
    W, H, nf = 1680, 1050, 12
    n = W * H
    rs = np.random.RandomState(8)
    base = rs.randint(0, 256, n).astype(np.int16)
    fr = np.clip(base[None] + rs.randint(-6, 7, (nf, n)), 0, 255).astype(np.uint8)
    fr[6:, 100000:140000] = 255
    mu, s6 = np.clip(base, 0, 255).astype(np.uint8), rs.randint(0, 12, n).astype(np.uint8)
    buf = fr.reshape(-1)
    F = torch.from_numpy(buf).to(DEV)
    M, S = model_tensors(mu, s6)
    jobs = [(i * n, max(i - 2, 0) * n) for i in range(nf)]
    got = check(F, buf, jobs, n, mu, s6, M, S, stride=(n + 15) & ~15, start=np.zeros((6, n), np.uint32))
    assert got[1, 100000:140000].min() == 6  # (the patch is saturated in the last six frames)


def test_nothing_to_do_and_the_argument_refusals():
    L = _lib.lib()
    buf = torch.full((8192,), 0x5A, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    assert p % 16 == 0
    ok = dict(frames=p, frames_bytes=4096, mu=p, sigma6=p, jobs=p, njobs=1, frame_bytes=64, planes=p + 4096, plane_stride=64, status=p + 2048,
              stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.abub_pixel_activity_dev(a["frames"], a["frames_bytes"], a["mu"], a["sigma6"], a["jobs"], a["njobs"], a["frame_bytes"],
                                         a["planes"], a["plane_stride"], a["status"], a["stream"])

    for kw in (dict(frames=None), dict(jobs=None), dict(planes=None), dict(status=None), dict(mu=None), dict(sigma6=None), dict(njobs=-1),
               dict(frame_bytes=0), dict(frame_bytes=(1 << 32) - 1, plane_stride=1 << 32), dict(plane_stride=60), dict(plane_stride=66),
               dict(planes=p + 4100), dict(jobs=p + 4), dict(status=p + 2050)):
        assert call(**kw) == E_INVALID, kw
        assert b"abub_pixel_activity_dev" in L.abub_last_error(), kw
    assert call(njobs=0) == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == 0x5A).all(), "a refused or empty call wrote something"
