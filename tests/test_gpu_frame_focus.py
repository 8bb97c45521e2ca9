"""abub_frame_focus_cells_dev (hip.frame_focus_cells) bit for bit against the host definition (host.focus_cells_host) and the
numpy restatement (tests/focusref.py): the sizes and contents of tests/test_focus_abi.py, so 130 x 130 where the ring is the
frame's edge, an origin at every residue mod 4 and grids of 2 x 1, 1 x 2 and 2 x 2 cells that share ring pixels; every
residue mod 16 of the frame's and the model's offset and of x0; both ways the kernel fills its tiles, up to the bounds
between them; the job list reversed and one job per call; 70,000 jobs
(more than one grid can index); jobs that run past their buffers; canaries round what the call writes; a full-size frame on
the R = 8 grid; and, cell by cell, the clipped pixels against abub_frame_light_cells_dev's two counts."""
import numpy as np
import pytest
import torch

import fieldref
import focusref
from autobub3hs_amd import hip, host
from test_focus_abi import C, N, focus_contents, focus_sizes
from test_gpu_frame_field import pack

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def check(pairs, x0, y0, ncx, ncy, **kw):
    h, w = pairs[0][0].shape
    fr, mu, jobs = pack(pairs, **kw)
    status, rec = hip.frame_focus_cells(fr, mu, jobs, w, h, x0, y0, ncx, ncy)
    assert not status.any() and rec.dtype == np.int32 and rec.shape == (len(pairs), ncy, ncx, 5)
    for k, (p, m) in enumerate(pairs):
        assert np.array_equal(rec[k], host.focus_cells_host(p, m, x0, y0, ncx, ncy)), (w, h, k)
        assert np.array_equal(rec[k], focusref.records(p, m, x0, y0, ncx, ncy)), (w, h, k)
    return rec


def test_kernel_against_the_definition_at_its_sizes():
    for w, h, x0, y0, ncx, ncy in focus_sizes():
        rs = np.random.RandomState(5000 + w)
        rs.randint(0, 256, (h, w))  # (the model plane of sigma6 in the definition's test: the same contents follow)
        rec = check(focus_contents(w, h, rs), x0, y0, ncx, ncy)
        assert np.array_equal(rec[1][..., 0].astype(np.int64) + rec[1][..., 1], rec[1][..., 2].astype(np.int64) + rec[1][..., 3])  # p = m
        assert (rec[2][..., 2:4] <= 0).all()  # p = 255 - m
        assert (rec[3] == [1065369600, 0, 1065369600, 0, N]).all()  # the stripes: the largest record
        assert (rec[4] == [0, 1065369600, 0, 1065369600, N]).all()
        assert not rec[5][..., 2:4].any()  # a flat model


def test_every_residue_of_the_offsets_and_of_x0():
    """the frame at every offset mod 16 against the model at every offset mod 16: 256 jobs of one size, all the same
    record; an odd width, so the rows themselves begin at every residue; then x0 at every residue mod 16"""
    w, h = C + 19, C + 4
    rs = np.random.RandomState(9)
    p, m = rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)
    n, step = w * h, (w * h + 31) // 16 * 16
    fr, mu = np.full(16 * step + 16, 0xEE, np.uint8), np.full(16 * step + 16, 0x11, np.uint8)
    for r in range(16):
        fr[r * step + r:r * step + r + n], mu[r * step + r:r * step + r + n] = p.reshape(-1), m.reshape(-1)
    jobs = [(a * step + a, b * step + b) for a in range(16) for b in range(16)]
    d_fr, d_mu = torch.from_numpy(fr).to(DEV), torch.from_numpy(mu).to(DEV)
    for x0 in (1, 4):
        status, rec = hip.frame_focus_cells(d_fr, d_mu, jobs, w, h, x0, 1, 1, 1)
        want = focusref.records(p, m, x0, 1, 1, 1)
        assert not status.any() and all(np.array_equal(s, want) for s in rec), x0
    for x0 in range(1, 19):  # (18: the ring ends where the row ends)
        status, rec = hip.frame_focus_cells(d_fr, d_mu, jobs[:1] + jobs[17:18], w, h, x0, 2, 1, 1)
        assert not status.any() and all(np.array_equal(s, focusref.records(p, m, x0, 2, 1, 1)) for s in rec), x0
    # ... and the buffers themselves at an odd address, their sizes exact: the last ring ends where the buffer ends
    d_fr, d_mu = torch.from_numpy(np.concatenate([[0, 0, 0], p.reshape(-1)]).astype(np.uint8)).to(DEV), torch.from_numpy(
        np.concatenate([[0], m.reshape(-1)]).astype(np.uint8)).to(DEV)
    status, rec = hip.frame_focus_cells(d_fr[3:], d_mu[1:], [(0, 0)], w, h, 18, 3, 1, 1)
    assert not status.any() and np.array_equal(rec[0], focusref.records(p, m, 18, 3, 1, 1))


def test_both_tile_fills_up_to_the_bounds_between_them():
    """a block whose tile has three bytes of the stream in front of it and four behind it fills it without a test per load,
    every other block with sh_load4: a frame that is one tile high, so the tile begins x0 - 1 bytes into the stream and ends
    w - x0 - 131 bytes before its end, with x0 from the first fill's side of either bound to the other's; the buffers are
    exactly the streams, at odd addresses"""
    w, h = C + 24, C + 2
    rs = np.random.RandomState(17)
    p, m = rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)
    d_fr = torch.from_numpy(np.concatenate([[9, 9, 9], p.reshape(-1)]).astype(np.uint8)).to(DEV)[3:]
    d_mu = torch.from_numpy(np.concatenate([[7], m.reshape(-1)]).astype(np.uint8)).to(DEV)[1:]
    for x0 in range(1, w - C):  # 1 .. 23: without a test from 4 (three bytes in front) to 17 (17 + 131 + 4 = w), the bounds themselves
        status, rec = hip.frame_focus_cells(d_fr, d_mu, [(0, 0)], w, h, x0, 1, 1, 1)
        assert not status.any() and np.array_equal(rec[0], focusref.records(p, m, x0, 1, 1, 1)), x0
    # two tiles high: the upper row of cells ends far from the stream's end, the lower one at it
    w, h = 2 * C + 7, 2 * C + 2
    p, m = rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)
    for x0 in (1, 3, 4, 6):
        status, rec = hip.frame_focus_cells(torch.from_numpy(p).to(DEV), torch.from_numpy(m).to(DEV), [(0, 0)], w, h, x0, 1, 2, 2)
        assert not status.any() and np.array_equal(rec[0], focusref.records(p, m, x0, 1, 2, 2)), x0


def test_the_order_of_the_jobs_does_not_matter():
    w, h, grid = 2 * C + 13, C + 11, (5, 7, 2, 1)
    rs = np.random.RandomState(31)
    pairs = [(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)) for _ in range(5)]
    fr, mu, jobs = pack(pairs, align=16)
    _, rec = hip.frame_focus_cells(fr, mu, jobs, w, h, *grid)
    status, back = hip.frame_focus_cells(fr, mu, jobs[::-1], w, h, *grid)
    assert not status.any() and np.array_equal(back[::-1], rec)
    for k, job in enumerate(jobs):
        _, one = hip.frame_focus_cells(fr, mu, [job], w, h, *grid)
        assert np.array_equal(one[0], rec[k])
    for k, (p, m) in enumerate(pairs):
        assert np.array_equal(rec[k], focusref.records(p, m, *grid))


def test_seventy_thousand_jobs():
    """more jobs than a grid dimension holds (65,535): blocks take several jobs each.  The jobs alias three frames and three
    models of 130 x 130, one cell each, every pairing"""
    n, s = 70000, C + 2
    rs = np.random.RandomState(3)
    p, m = rs.randint(0, 256, (3, s, s)).astype(np.uint8), rs.randint(0, 256, (3, s, s)).astype(np.uint8)
    k = np.arange(n)
    jobs = np.stack([(k % 3) * s * s, (k // 3 % 3) * s * s], axis=1)
    status, rec = hip.frame_focus_cells(torch.from_numpy(p).to(DEV), torch.from_numpy(m).to(DEV), jobs, s, s, 1, 1, 1, 1)
    want = np.array([[focusref.records(p[a], m[b], 1, 1, 1, 1) for b in range(3)] for a in range(3)])
    assert not status.any() and np.array_equal(rec, want[k % 3, k // 3 % 3])


def test_jobs_past_their_buffers_and_canaries():
    """job 1 runs past frames_bytes by one byte, job 3 past model_bytes, jobs 5 and 6 have an offset beyond any buffer: status
    set, record zero, nothing of them read; their neighbours are intact.  status and rec lie inside larger tensors whose
    other words must keep their values."""
    w, h, grid = 2 * C + 10, C + 9, (6, 5, 2, 1)
    n, words = w * h, 2 * 5  # two cells
    rs = np.random.RandomState(41)
    pairs = [(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)) for _ in range(4)]
    fr, mu, jobs = pack(pairs, align=16)
    end = 4 * ((n + 15) // 16 * 16)
    jobs = [jobs[0], (end - n + 1, 0), jobs[1], (0, end - n + 1), jobs[2], (1 << 40, 0), (0, (1 << 64) - 1), jobs[3]]
    nj = len(jobs)
    status_all = torch.full((nj + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rec_all = torch.full((nj * words + 9,), 0x01234567, dtype=torch.int32, device=DEV)
    status, rec = hip.frame_focus_cells(fr, mu, jobs, w, h, *grid, frames_bytes=end, model_bytes=end, status=status_all[4:4 + nj],
                                        rec=rec_all[5:5 + nj * words])  # (an odd word: rec need only be 4-byte aligned)
    assert list(status) == [0, focusref.E_RANGE, 0, focusref.E_RANGE, 0, focusref.E_RANGE, focusref.E_RANGE, 0]
    for k, pair in zip((0, 2, 4, 7), pairs):
        assert np.array_equal(rec[k], focusref.records(pair[0], pair[1], *grid)), k
    assert not rec[[1, 3, 5, 6]].any()
    st, rc = status_all.cpu().numpy(), rec_all.cpu().numpy()
    assert (st[:4] == 0x5A5A5A5A).all() and (st[4 + nj:] == 0x5A5A5A5A).all()
    assert (rc[:5] == 0x01234567).all() and (rc[5 + nj * words:] == 0x01234567).all()
    # the same list one byte more generous: jobs 1 and 3 now end exactly where their buffers end, and are read
    fr2, mu2 = torch.cat([fr[:end], fr[:1]]), torch.cat([mu[:end], mu[:1]])
    status, rec = hip.frame_focus_cells(fr2, mu2, jobs[:4], w, h, *grid)
    assert not status.any()
    a, b = fr2.cpu().numpy(), mu2.cpu().numpy()
    assert np.array_equal(rec[1], focusref.records(a[end - n + 1:end + 1].reshape(h, w), b[:n].reshape(h, w), *grid))
    assert np.array_equal(rec[3], focusref.records(a[:n].reshape(h, w), b[end - n + 1:end + 1].reshape(h, w), *grid))


def test_a_full_size_frame_on_the_grid_of_the_largest_radius():
    """1680 x 1050 on the grid of R = 8: 13 x 8 cells from (8, 13), in one launch"""
    rs = np.random.RandomState(77)
    w, h = 1680, 1050
    ncx, ncy, x0, y0 = fieldref.grid(w, h, 8)
    assert (ncx, ncy, x0, y0) == (13, 8, 8, 13) == hip.field_grid(w, h, 8)
    check([(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8))], x0, y0, ncx, ncy)


def test_every_cell_s_clipped_pixels_against_the_light_kernel():
    """an existing kernel, another decomposition: n_clip is abub_frame_light_cells_dev's n_zero + n_sat on the same grid"""
    R, w, h = 4, 2 * C + 2 * 4 + 1, 2 * C + 2 * 4 + 2
    ncx, ncy, x0, y0 = fieldref.grid(w, h, R)
    rs = np.random.RandomState(13)
    p, m = rs.choice(np.array([0, 1, 77, 200, 254, 255], np.uint8), (h, w)), rs.randint(0, 256, (h, w)).astype(np.uint8)
    fr, mu, jobs = pack([(p, m)])
    status, rec = hip.frame_focus_cells(fr, mu, jobs, w, h, x0, y0, ncx, ncy)
    status2, light = hip.frame_light_cells(fr, mu, jobs, w, h, x0, y0, ncx, ncy)
    assert not status.any() and not status2.any() and rec[..., 4].min() > N // 4
    assert np.array_equal(rec[0, :, :, 4].astype(np.int64), light[0, :, :, 4].astype(np.int64) + light[0, :, :, 5])
