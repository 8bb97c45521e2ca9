"""abub_frame_noise_cells_dev (hip.frame_noise_cells) bit for bit against the host definition (host.noise_cells_host) and the
numpy restatement (tests/noiseref.py): the sizes and contents of tests/test_noise_abi.py; each of the three streams at every
offset residue mod 16 while the other two stay, and all three together; x0 over 0 .. 19 on an odd width; buffers at an odd
address that end where the last cell ends; the job list reversed and one job per call; 70,000 jobs (more than one grid can
index); jobs that run past each of the three buffers; canaries round what the call writes; a full-size frame on the R = 8
grid; and, cell by cell, three existing kernels: the field's entry at (0, 0), the light's sums and the frame statistics'
n_moved of the crops."""
import numpy as np
import pytest
import torch

import fieldref
import noiseref
from autobub3hs_amd import hip, host
from test_noise_abi import C, N, noise_contents, noise_sizes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def pack(triples, align=1, lead=0):
    """[(frame, reference frame, sigma6)] of one size -> (frames u8 tensor, sigma6 u8 tensor, jobs): frame k at the next
    multiple of `align` behind `lead` bytes, its reference frame behind all the frames, its plane where its frame is"""
    n, k = triples[0][0].size, len(triples)
    step = (n + align - 1) // align * align
    fr, sg = np.zeros(lead + step * 2 * k, np.uint8), np.zeros(lead + step * k, np.uint8)
    jobs = []
    for q, (p, r, s) in enumerate(triples):
        at, ref = lead + q * step, lead + (k + q) * step
        fr[at:at + n], fr[ref:ref + n], sg[at:at + n] = p.reshape(-1), r.reshape(-1), s.reshape(-1)
        jobs.append((at, ref, at))
    return torch.from_numpy(fr).to(DEV), torch.from_numpy(sg).to(DEV), jobs


def check(triples, x0, y0, ncx, ncy, **kw):
    h, w = triples[0][0].shape
    fr, sg, jobs = pack(triples, **kw)
    status, rec = hip.frame_noise_cells(fr, sg, jobs, w, h, x0, y0, ncx, ncy)
    assert not status.any() and rec.dtype == np.int32 and rec.shape == (len(triples), ncy, ncx, 6)
    for k, (p, r, s) in enumerate(triples):
        assert np.array_equal(rec[k], host.noise_cells_host(p, r, s, x0, y0, ncx, ncy)), (w, h, x0, k)
        assert np.array_equal(rec[k], noiseref.records(p, r, s, x0, y0, ncx, ncy)), (w, h, x0, k)
    return rec


def test_kernel_against_the_definition_at_its_sizes():
    for w, h, x0, y0, ncx, ncy in noise_sizes():
        rec = check(noise_contents(w, h, np.random.RandomState(5000 + w + x0)), x0, y0, ncx, ncy)
        assert (rec[1] == [0, N, 255 * N, 1065369600, 255 * N, 1065369600]).all()  # 255 against 0 inside s = 255: the largest record
        assert (rec[2] == [0, N, -255 * N, 1065369600, 255 * N, 1065369600]).all()
        assert (rec[5][..., 0] == N // 2).all() and (rec[6][..., 0] == N // 2).all() and not rec[7][..., [0, 2, 3, 4, 5]].any()


def test_the_reference_may_be_the_frame_itself():
    """ref == cur, the same bytes read through two streams: d = 0, and only the clipped pixels are counted"""
    rs = np.random.RandomState(8)
    p = rs.choice(np.array([0, 1, 90, 254, 255], np.uint8), (C + 3, C + 6))
    s = rs.randint(0, 256, p.shape).astype(np.uint8)
    status, rec = hip.frame_noise_cells(torch.from_numpy(p).to(DEV), torch.from_numpy(s).to(DEV), [(0, 0, 0)], C + 6, C + 3, 5, 2, 1, 1)
    assert not status.any() and np.array_equal(rec[0], noiseref.records(p, p, s, 5, 2, 1, 1))
    assert not rec[0][..., [0, 2, 3, 4, 5]].any() and rec[0][0, 0, 1] == ((p[2:2 + C, 5:5 + C] % 255) == 0).sum()


def test_every_residue_of_the_three_offsets_and_of_x0():
    """an odd width, so the rows themselves begin at every residue; 16 copies of each stream, copy a at an offset of residue
    a mod 16: each stream through every residue while the other two stay at 0, 5 and 10, then all three together; then x0
    over 0 .. 19 (19: the cell ends where the row ends); then the buffers themselves at odd addresses, their sizes exact"""
    w, h = C + 19, C + 2
    rs = np.random.RandomState(9)
    p, r, s = (rs.randint(0, 256, (h, w)).astype(np.uint8) for _ in range(3))
    s[:, ::3] = 0
    n, step = w * h, (w * h + 31) // 16 * 16
    fr, sg = np.full(32 * step + 16, 0xEE, np.uint8), np.full(16 * step + 16, 0x11, np.uint8)
    for a in range(16):
        fr[a * step + a:a * step + a + n], sg[a * step + a:a * step + a + n] = p.reshape(-1), s.reshape(-1)
        fr[(16 + a) * step + a:(16 + a) * step + a + n] = r.reshape(-1)
    cur, ref, mod = (lambda a: a * step + a), (lambda a: (16 + a) * step + a), (lambda a: a * step + a)
    jobs = [(cur(a), ref(5), mod(10)) for a in range(16)] + [(cur(0), ref(a), mod(10)) for a in range(16)]
    jobs += [(cur(0), ref(5), mod(a)) for a in range(16)] + [(cur(a), ref(a), mod(a)) for a in range(16)]
    d_fr, d_sg = torch.from_numpy(fr).to(DEV), torch.from_numpy(sg).to(DEV)
    for x0 in (0, 3):
        status, rec = hip.frame_noise_cells(d_fr, d_sg, jobs, w, h, x0, 1, 1, 1)
        want = noiseref.records(p, r, s, x0, 1, 1, 1)
        assert not status.any() and len(rec) == 64 and all(np.array_equal(v, want) for v in rec), x0
    for x0 in range(20):
        status, rec = hip.frame_noise_cells(d_fr, d_sg, [jobs[0], jobs[21], jobs[63]], w, h, x0, 2, 1, 1)
        assert not status.any() and all(np.array_equal(v, noiseref.records(p, r, s, x0, 2, 1, 1)) for v in rec), x0
    both = np.concatenate([[0, 0, 0], p.reshape(-1), r.reshape(-1)]).astype(np.uint8)
    d_fr, d_sg = torch.from_numpy(both).to(DEV), torch.from_numpy(np.concatenate([[0], s.reshape(-1)]).astype(np.uint8)).to(DEV)
    status, rec = hip.frame_noise_cells(d_fr[3:], d_sg[1:], [(0, n, 0), (n, 0, 0)], w, h, 19, 2, 1, 1)
    assert not status.any() and np.array_equal(rec[0], noiseref.records(p, r, s, 19, 2, 1, 1))
    assert np.array_equal(rec[1], noiseref.records(r, p, s, 19, 2, 1, 1))


def test_the_order_of_the_jobs_does_not_matter():
    w, h, grid = 2 * C + 13, C + 11, (5, 7, 2, 1)
    rs = np.random.RandomState(31)
    triples = [tuple(rs.randint(0, 256, (h, w)).astype(np.uint8) for _ in range(3)) for _ in range(5)]
    fr, sg, jobs = pack(triples, align=16)
    _, rec = hip.frame_noise_cells(fr, sg, jobs, w, h, *grid)
    status, back = hip.frame_noise_cells(fr, sg, jobs[::-1], w, h, *grid)
    assert not status.any() and np.array_equal(back[::-1], rec)
    for k, job in enumerate(jobs):
        _, one = hip.frame_noise_cells(fr, sg, [job], w, h, *grid)
        assert np.array_equal(one[0], rec[k])
    for k, (p, r, s) in enumerate(triples):
        assert np.array_equal(rec[k], noiseref.records(p, r, s, *grid))


def test_seventy_thousand_jobs():
    """more jobs than a grid dimension holds (65,535): blocks take several jobs each.  The jobs alias three frames of one
    cell each, as the frame, as the reference and as the plane, every combination"""
    n = 70000
    f = np.random.RandomState(3).randint(0, 256, (3, C, C)).astype(np.uint8)
    k = np.arange(n)
    jobs = np.stack([(k % 3) * N, (k // 3 % 3) * N, (k // 9 % 3) * N], axis=1)
    d = torch.from_numpy(f).to(DEV)
    status, rec = hip.frame_noise_cells(d, d, jobs, C, C, 0, 0, 1, 1)
    want = np.array([[[noiseref.records(f[a], f[b], f[c], 0, 0, 1, 1) for c in range(3)] for b in range(3)] for a in range(3)])
    assert not status.any() and np.array_equal(rec, want[k % 3, k // 3 % 3, k // 9 % 3])


def test_jobs_past_their_buffers_and_canaries():
    """jobs 1, 3 and 5 run past the end of the frames (as the frame, as the reference) and of the planes by one byte, jobs 7
    to 9 have an offset of UINT64_MAX in each place, job 10 one beyond any buffer: status set, record zero, nothing of them
    read; their neighbours are intact.  status and rec lie inside larger tensors whose other words must keep their values."""
    w, h, grid = 2 * C + 10, C + 9, (6, 5, 2, 1)
    n, words = w * h, 2 * 6  # two cells
    rs = np.random.RandomState(41)
    triples = [tuple(rs.randint(0, 256, (h, w)).astype(np.uint8) for _ in range(3)) for _ in range(4)]
    fr, sg, jobs = pack(triples, align=16)
    step = (n + 15) // 16 * 16
    fend, mend, top = 8 * step, 4 * step, (1 << 64) - 1
    jobs = [jobs[0], (fend - n + 1, 0, 0), jobs[1], (0, fend - n + 1, 0), jobs[2], (0, step, mend - n + 1), jobs[3], (top, 0, 0),
            (0, top, 0), (0, 0, top), (1 << 40, 0, 0)]
    nj = len(jobs)
    status_all = torch.full((nj + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rec_all = torch.full((nj * words + 9,), 0x01234567, dtype=torch.int32, device=DEV)
    status, rec = hip.frame_noise_cells(fr, sg, jobs, w, h, *grid, frames_bytes=fend, model_bytes=mend, status=status_all[4:4 + nj],
                                        rec=rec_all[5:5 + nj * words])  # (an odd word: rec need only be 4-byte aligned)
    E = noiseref.E_RANGE
    assert list(status) == [0, E, 0, E, 0, E, 0, E, E, E, E]
    for k, t in zip((0, 2, 4, 6), triples):
        assert np.array_equal(rec[k], noiseref.records(*t, *grid)), k
    assert not rec[[1, 3, 5, 7, 8, 9, 10]].any()
    st, rc = status_all.cpu().numpy(), rec_all.cpu().numpy()
    assert (st[:4] == 0x5A5A5A5A).all() and (st[4 + nj:] == 0x5A5A5A5A).all()
    assert (rc[:5] == 0x01234567).all() and (rc[5 + nj * words:] == 0x01234567).all()
    # the same list one byte more generous: jobs 1, 3 and 5 now end exactly where their buffers end, and are read
    fr2, sg2 = torch.cat([fr[:fend], fr[:1]]), torch.cat([sg[:mend], sg[:1]])
    status, rec = hip.frame_noise_cells(fr2, sg2, jobs[:6], w, h, *grid)
    assert not status.any()
    a, b = fr2.cpu().numpy(), sg2.cpu().numpy()
    img = lambda buf, at: buf[at:at + n].reshape(h, w)  # noqa: E731
    assert np.array_equal(rec[1], noiseref.records(img(a, fend - n + 1), img(a, 0), img(b, 0), *grid))
    assert np.array_equal(rec[3], noiseref.records(img(a, 0), img(a, fend - n + 1), img(b, 0), *grid))
    assert np.array_equal(rec[5], noiseref.records(img(a, 0), img(a, step), img(b, mend - n + 1), *grid))


def test_a_full_size_frame_on_the_grid_of_the_largest_radius():
    """1680 x 1050 on the grid of R = 8: 13 x 8 cells from (8, 13); noise of sigma 3 around a ramp, so that some pixels are
    over and most are not"""
    rs = np.random.RandomState(77)
    w, h = 1680, 1050
    ncx, ncy, x0, y0 = fieldref.grid(w, h, 8)
    assert (ncx, ncy, x0, y0) == (13, 8, 8, 13) == hip.field_grid(w, h, 8)
    back = np.add.outer(np.arange(h), np.arange(w)) % 251
    noisy = lambda: np.clip(np.rint(back + 3 * rs.standard_normal((h, w))), 0, 255).astype(np.uint8)  # noqa: E731
    rec = check([(noisy(), noisy(), rs.randint(6, 19, (h, w)).astype(np.uint8))], x0, y0, ncx, ncy)
    assert (rec[0][..., 0] > 0).all() and (rec[0][..., 0] < N // 4).all() and (rec[0][..., 1] > 0).any()


def test_every_cell_against_three_existing_kernels():
    """other kernels, other decompositions: sad is abub_frame_shift_cells_dev's entry at (0, 0) with the reference frame
    passed as its mu; s2_all = sum p^2 + sum r^2 - 2 sum p r from three words of abub_frame_light_cells_dev (p against r, and
    r against itself); n_over is abub_frame_stats_dev's n_moved of the cell's crops as frames of their own"""
    Rf, w, h = 4, 2 * C + 2 * 4 + 1, 2 * C + 2 * 4 + 2
    ncx, ncy, x0, y0 = fieldref.grid(w, h, Rf)
    rs = np.random.RandomState(13)
    p = rs.choice(np.array([0, 1, 77, 200, 254, 255], np.uint8), (h, w))
    r = np.clip(p.astype(np.int64) + rs.randint(-30, 31, (h, w)), 0, 255).astype(np.uint8)
    s = rs.randint(0, 31, (h, w)).astype(np.uint8)
    fr, sg, jobs = pack([(p, r, s)])
    _, rec = hip.frame_noise_cells(fr, sg, jobs, w, h, x0, y0, ncx, ncy)
    assert np.array_equal(rec[0], noiseref.records(p, r, s, x0, y0, ncx, ncy))
    cur, ref = jobs[0][0], jobs[0][1]
    status, sad = hip.frame_shift_cells(fr, fr, [(cur, ref)], w, h, Rf)
    assert not status.any() and np.array_equal(sad[0, :, :, Rf, Rf], rec[0, :, :, 4])
    status, light = hip.frame_light_cells(fr, fr, [(cur, ref), (ref, ref)], w, h, x0, y0, ncx, ncy)
    light = light.astype(np.int64)
    assert not status.any() and np.array_equal(light[0, :, :, 1] + light[1, :, :, 1] - 2 * light[0, :, :, 2], rec[0, :, :, 5])
    assert np.array_equal(light[0, :, :, 3], rec[0, :, :, 4])
    cells = [(cx, cy) for cy in range(ncy) for cx in range(ncx)]
    crop = lambda a: np.stack([a[y0 + C * cy:y0 + C * (cy + 1), x0 + C * cx:x0 + C * (cx + 1)] for cx, cy in cells])  # noqa: E731
    k = len(cells)
    both = torch.from_numpy(np.concatenate([crop(p), crop(r)])).to(DEV)
    planes = torch.from_numpy(crop(s)).to(DEV)
    res = hip.frame_stats(both, [(q * N, (k + q) * N, q * N) for q in range(k)], N, mu=planes, sigma6=planes)
    col = {name: q for q, name in enumerate(hip.STAT_COLUMNS)}
    for q, (cx, cy) in enumerate(cells):
        assert res[q, col["status"]] == 0 and int(res[q, col["flags"]]) & 2
        assert int(res[q, col["n_moved"]]) == int(rec[0, cy, cx, 0]), (cx, cy)
