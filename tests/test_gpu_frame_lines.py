"""abub_frame_lines_dev (hip.frame_lines) bit for bit against the host definition (host.lines_host) and the numpy restatement
(tests/linesref.py): the shapes and contents of tests/test_lines_abi.py; the two longest lines; each of the three streams at
every offset residue mod 16 while the other two stay, and all three together, on an odd width; buffers at odd addresses that
end where the last frame ends; the job list reversed and one job per call; 70,000 jobs (more than one grid can index); jobs
that run past each of the three buffers; both outputs preset to 0x5A inside canaries; the reference the frame itself; a
full-size frame; and three cross-checks against existing kernels."""
import numpy as np
import pytest
import torch

import linesref
from autobub3hs_amd import hip, host
from test_lines_abi import lines_contents, lines_shapes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NONE = hip.STAT_NONE
E_RANGE = hip.SHIFT_E_RANGE


def pack(triples, align=1, lead=0):
    """[(frame, mu, reference frame or None)] of one shape -> (frames u8 tensor, mu u8 tensor, jobs): frame k at the next
    multiple of `align` behind `lead` bytes, its reference frame behind all the frames, its plane where its frame is"""
    n, k = triples[0][0].size, len(triples)
    step = (n + align - 1) // align * align
    fr, mu = np.zeros(lead + step * 2 * k, np.uint8), np.zeros(lead + step * k, np.uint8)
    jobs = []
    for q, (p, m, r) in enumerate(triples):
        at, ref = lead + q * step, lead + (k + q) * step
        fr[at:at + n], mu[at:at + n] = p.reshape(-1), m.reshape(-1)
        if r is not None:
            fr[ref:ref + n] = r.reshape(-1)
        jobs.append((at, NONE if r is None else ref, at))
    return torch.from_numpy(fr).to(DEV), torch.from_numpy(mu).to(DEV), jobs


def want_of(p, m, r):
    return [a.astype(np.uint32) for a in linesref.records(p, m, r)]


def check(triples, **kw):
    h, w = triples[0][0].shape
    fr, mu, jobs = pack(triples, **kw)
    status, rows, cols = hip.frame_lines(fr, mu, jobs, w, h)
    assert not status.any() and rows.dtype == cols.dtype == np.uint32
    assert rows.shape == (len(triples), h, 5) and cols.shape == (len(triples), w, 3)
    for k, (p, m, r) in enumerate(triples):
        hr, hc = host.lines_host(p, m, r)
        wr, wc = want_of(p, m, r)
        assert np.array_equal(rows[k], hr) and np.array_equal(cols[k], hc), (w, h, k)
        assert np.array_equal(rows[k], wr) and np.array_equal(cols[k], wc), (w, h, k)
    return rows, cols


@pytest.mark.parametrize("w,h", lines_shapes())
def test_kernel_against_the_definition_at_its_shapes(w, h):
    rows, cols = check(lines_contents(w, h, np.random.RandomState(7000 + w + h)))
    assert (rows[1][:, [0, 1, 2, 4]] == [255 * w, 255 * w, w, w]).all() and (cols[2][:, 1:] == [255 * h, h]).all()
    assert (rows[3][:, 4] == w).all() and (rows[4][:, 4] == w - 1).all() and not rows[6][:, 3:].any()


@pytest.mark.parametrize("w,h", [(65535, 1), (1, 65535)])
def test_the_longest_lines(w, h):
    """all 255 against mu = 0: 16,711,425 in a row word, in a column word"""
    full, none = np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    rows, cols = check([(full, none, full), (full, none, None)])
    assert max(rows[0][:, 1].max(), cols[0][:, 1].max()) == 16711425 and (rows[1][:, 3:] == 0).all()


def test_the_reference_may_be_the_frame_itself():
    """ref == cur, the same bytes read through two streams: n_same = W and word 3 = 0"""
    rs = np.random.RandomState(8)
    p = rs.choice(np.array([0, 1, 90, 254, 255], np.uint8), (131, 139))
    m = rs.randint(0, 256, p.shape).astype(np.uint8)
    status, rows, cols = hip.frame_lines(torch.from_numpy(p).to(DEV), torch.from_numpy(m).to(DEV), [(0, 0, 0)], 139, 131)
    wr, wc = want_of(p, m, p)
    assert not status.any() and np.array_equal(rows[0], wr) and np.array_equal(cols[0], wc)
    assert (rows[0][:, 4] == 139).all() and not rows[0][:, 3].any()


def test_every_residue_of_the_three_offsets():
    """an odd width, so the rows themselves begin at every residue; 16 copies of each stream, copy a at an offset of residue
    a mod 16: each stream through every residue while the other two stay at 0, 5 and 10, then all three together; then the
    buffers themselves at odd addresses, their sizes exact: they end where the last frame ends"""
    w, h = 147, 21
    rs = np.random.RandomState(9)
    p, r, m = (rs.randint(0, 256, (h, w)).astype(np.uint8) for _ in range(3))
    r[::3] = p[::3]
    n, step = w * h, (w * h + 31) // 16 * 16
    fr, mu = np.full(32 * step + 16, 0xEE, np.uint8), np.full(16 * step + 16, 0x11, np.uint8)
    for a in range(16):
        fr[a * step + a:a * step + a + n], mu[a * step + a:a * step + a + n] = p.reshape(-1), m.reshape(-1)
        fr[(16 + a) * step + a:(16 + a) * step + a + n] = r.reshape(-1)
    cur, ref, mod = (lambda a: a * step + a), (lambda a: (16 + a) * step + a), (lambda a: a * step + a)
    jobs = [(cur(a), ref(5), mod(10)) for a in range(16)] + [(cur(0), ref(a), mod(10)) for a in range(16)]
    jobs += [(cur(0), ref(5), mod(a)) for a in range(16)] + [(cur(a), ref(a), mod(a)) for a in range(16)]
    status, rows, cols = hip.frame_lines(torch.from_numpy(fr).to(DEV), torch.from_numpy(mu).to(DEV), jobs, w, h)
    wr, wc = want_of(p, m, r)
    assert not status.any() and len(rows) == 64
    assert all(np.array_equal(v, wr) for v in rows) and all(np.array_equal(v, wc) for v in cols)
    both = np.concatenate([[0, 0, 0], p.reshape(-1), r.reshape(-1)]).astype(np.uint8)
    d_fr, d_mu = torch.from_numpy(both).to(DEV), torch.from_numpy(np.concatenate([[0], m.reshape(-1)]).astype(np.uint8)).to(DEV)
    status, rows, cols = hip.frame_lines(d_fr[3:], d_mu[1:], [(0, n, 0), (n, 0, 0), (n, NONE, 0)], w, h)
    assert not status.any()
    for k, t in enumerate(((p, m, r), (r, m, p), (r, m, None))):
        wr, wc = want_of(*t)
        assert np.array_equal(rows[k], wr) and np.array_equal(cols[k], wc), k


def test_the_order_of_the_jobs_does_not_matter():
    w, h = 269, 141
    rs = np.random.RandomState(31)
    triples = [tuple(rs.randint(0, 256, (h, w)).astype(np.uint8) for _ in range(3)) for _ in range(5)]
    fr, mu, jobs = pack(triples, align=16)
    _, rows, cols = hip.frame_lines(fr, mu, jobs, w, h)
    status, rback, cback = hip.frame_lines(fr, mu, jobs[::-1], w, h)
    assert not status.any() and np.array_equal(rback[::-1], rows) and np.array_equal(cback[::-1], cols)
    for k, job in enumerate(jobs):
        _, r1, c1 = hip.frame_lines(fr, mu, [job], w, h)
        assert np.array_equal(r1[0], rows[k]) and np.array_equal(c1[0], cols[k])
    for k, t in enumerate(triples):
        wr, wc = want_of(*t)
        assert np.array_equal(rows[k], wr) and np.array_equal(cols[k], wc)


def test_seventy_thousand_jobs():
    """more jobs than a grid dimension holds (65,535): blocks take several jobs each.  The jobs alias three frames of 8 x 4,
    as the frame, as the reference (or none) and as the plane, every combination"""
    n, w, h = 70000, 8, 4
    f = np.random.RandomState(3).randint(0, 256, (3, h, w)).astype(np.uint8)
    f[1, 2] = f[0, 2]
    k = np.arange(n)
    refs = np.array([0, w * h, 2 * w * h, NONE], np.uint64)
    jobs = np.stack([(k % 3 * w * h).astype(np.uint64), refs[k // 3 % 4], (k // 12 % 3 * w * h).astype(np.uint64)], axis=1)
    d = torch.from_numpy(f).to(DEV)
    status, rows, cols = hip.frame_lines(d, d, jobs, w, h)
    want = [[[want_of(f[a], f[c], None if b == 3 else f[b]) for c in range(3)] for b in range(4)] for a in range(3)]
    wr = np.array([[[v[0] for v in y] for y in x] for x in want])
    wc = np.array([[[v[1] for v in y] for y in x] for x in want])
    assert not status.any() and np.array_equal(rows, wr[k % 3, k // 3 % 4, k // 12 % 3]) and np.array_equal(cols, wc[k % 3, k // 3 % 4, k // 12 % 3])


def test_jobs_past_their_buffers_and_canaries():
    """jobs 1, 3 and 5 run past the end of the frames (as the frame, as the reference) and of the planes by one byte, jobs 7
    and 8 have an offset of UINT64_MAX as the frame and as the plane, job 9 one beyond any buffer: status set, records zero,
    nothing of them read; their neighbours are intact.  status, rows and cols lie inside larger tensors preset to 0x5A whose
    other words must keep their values."""
    w, h = 266, 137
    n = w * h
    rs = np.random.RandomState(41)
    triples = [tuple(rs.randint(0, 256, (h, w)).astype(np.uint8) for _ in range(3)) for _ in range(4)]
    fr, mu, jobs = pack(triples, align=16)
    step = (n + 15) // 16 * 16
    fend, mend, top = 8 * step, 4 * step, (1 << 64) - 1
    jobs = [jobs[0], (fend - n + 1, 0, 0), jobs[1], (0, fend - n + 1, 0), jobs[2], (0, step, mend - n + 1), jobs[3], (top, 0, 0),
            (0, 0, top), (1 << 40, 0, 0)]
    nj = len(jobs)
    fill = 0x5A5A5A5A
    status_all = torch.full((nj + 8,), fill, dtype=torch.int32, device=DEV)
    rows_all = torch.full((nj * h * 5 + 9,), fill, dtype=torch.int32, device=DEV)
    cols_all = torch.full((nj * w * 3 + 7,), fill, dtype=torch.int32, device=DEV)
    status, rows, cols = hip.frame_lines(fr, mu, jobs, w, h, frames_bytes=fend, model_bytes=mend, status=status_all[4:4 + nj],
                                         rows=rows_all[5:5 + nj * h * 5], cols=cols_all[3:3 + nj * w * 3])
    E = E_RANGE
    assert list(status) == [0, E, 0, E, 0, E, 0, E, E, E]
    for k, t in zip((0, 2, 4, 6), triples):
        wr, wc = want_of(t[0], t[1], t[2])
        assert np.array_equal(rows[k], wr) and np.array_equal(cols[k], wc), k
    assert not rows[[1, 3, 5, 7, 8, 9]].any() and not cols[[1, 3, 5, 7, 8, 9]].any()
    st, rw, cl = status_all.cpu().numpy(), rows_all.cpu().numpy(), cols_all.cpu().numpy()
    assert (st[:4] == fill).all() and (st[4 + nj:] == fill).all()
    assert (rw[:5] == fill).all() and (rw[5 + nj * h * 5:] == fill).all() and (cl[:3] == fill).all() and (cl[3 + nj * w * 3:] == fill).all()
    # the same list one byte more generous: jobs 1, 3 and 5 now end exactly where their buffers end, and are read
    fr2, mu2 = torch.cat([fr[:fend], fr[:1]]), torch.cat([mu[:mend], mu[:1]])
    status, rows, cols = hip.frame_lines(fr2, mu2, jobs[:6], w, h)
    assert not status.any()
    a, b = fr2.cpu().numpy(), mu2.cpu().numpy()
    img = lambda buf, at: buf[at:at + n].reshape(h, w)  # noqa: E731
    for k, t in ((1, (img(a, fend - n + 1), img(b, 0), img(a, 0))), (3, (img(a, 0), img(b, 0), img(a, fend - n + 1))),
                 (5, (img(a, 0), img(b, mend - n + 1), img(a, step)))):
        wr, wc = want_of(*t)
        assert np.array_equal(rows[k], wr) and np.array_equal(cols[k], wc), k


def test_a_full_size_frame():
    rs = np.random.RandomState(77)
    w, h = 1680, 1050
    back = np.add.outer(np.arange(h), np.arange(w)) % 251
    noisy = lambda: np.clip(np.rint(back + 3 * rs.standard_normal((h, w))), 0, 255).astype(np.uint8)  # noqa: E731
    a = noisy()
    b = noisy()
    b[700:] = a[700:]
    rows, _ = check([(a, np.clip(back, 0, 255).astype(np.uint8), b)])
    assert (rows[0][700:, 4] == w).all() and (rows[0][:700, 4] < w).all() and (rows[0][:, 2] > 0).any()


def test_the_sums_against_three_existing_kernels():
    """other kernels, other decompositions, on 256 x 128: the row words 0 summed are abub_frame_stats_dev's sum, the n_clip
    summed its n_zero + n_sat; the words 1 summed over each cell's rows and over its columns are the sum |p - mu| of
    abub_frame_light_cells_dev on the 2 x 1 grid at the origin"""
    w, h, C = 256, 128, 128
    rs = np.random.RandomState(13)
    p = rs.choice(np.array([0, 1, 77, 200, 254, 255], np.uint8), (h, w))
    m = rs.randint(0, 256, (h, w)).astype(np.uint8)
    fr, mu = torch.from_numpy(p).to(DEV), torch.from_numpy(m).to(DEV)
    status, rows, cols = hip.frame_lines(fr, mu, [(0, NONE, 0)], w, h)
    assert not status.any()
    rows, cols = rows[0].astype(np.int64), cols[0].astype(np.int64)
    res = hip.frame_stats(fr, [(0, 0, 0)], w * h, mu=mu, sigma6=mu)
    col = {name: q for q, name in enumerate(hip.STAT_COLUMNS)}
    assert res[0, col["status"]] == 0
    assert int(res[0, col["sum"]]) == rows[:, 0].sum() == cols[:, 0].sum()
    assert int(res[0, col["n_zero"]]) + int(res[0, col["n_sat"]]) == rows[:, 2].sum() == cols[:, 2].sum()
    status, light = hip.frame_light_cells(fr, mu, [(0, 0)], w, h, 0, 0, 2, 1)
    assert not status.any()
    dev = np.abs(p.astype(np.int64) - m.astype(np.int64))
    for cx in range(2):
        assert int(light[0, 0, cx, 3]) == cols[C * cx:C * (cx + 1), 1].sum() == dev[:, C * cx:C * (cx + 1)].sum()
    assert int(light[0, 0, :, 3].astype(np.int64).sum()) == rows[:, 1].sum()
