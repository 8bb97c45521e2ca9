"""abub_frame_shift_cells_dev (hip.frame_shift_cells) bit for bit against the numpy restatement (tests/fieldref.py): the sizes
and contents of tests/test_field_abi.py, so one cell without a margin, an origin at every residue mod 4, odd widths and grids
of 2 x 1, 2 x 2 and 3 x 1 cells; every radius; planted displacements; every residue mod 16 of the frame's and the model's
offset; the job list reversed and one job per call; 70,000 jobs (more than one grid can index); jobs that run past their
buffers; canaries round what the call writes; a full-size frame; and, cell by cell, abub_frame_shift_dev on the crops."""
import numpy as np
import pytest
import torch

import fieldref
from autobub3hs_amd import hip
from test_field_abi import C, RADII, field_contents, field_sizes, planted

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def pack(pairs, align=1, lead=0):
    """[(frame, model)] of one size -> (frames u8 tensor, mu u8 tensor, jobs): each plane at the next multiple of `align`
    behind `lead` bytes"""
    n = pairs[0][0].size
    step = (n + align - 1) // align * align
    fr, mu = np.zeros(lead + step * len(pairs), np.uint8), np.zeros(lead + step * len(pairs), np.uint8)
    jobs = []
    for k, (p, m) in enumerate(pairs):
        at = lead + k * step
        fr[at:at + n], mu[at:at + n] = p.reshape(-1), m.reshape(-1)
        jobs.append((at, at))
    return torch.from_numpy(fr).to(DEV), torch.from_numpy(mu).to(DEV), jobs


def check(pairs, R, **kw):
    h, w = pairs[0][0].shape
    fr, mu, jobs = pack(pairs, **kw)
    status, sad = hip.frame_shift_cells(fr, mu, jobs, w, h, R)
    ncx, ncy, _, _ = fieldref.grid(w, h, R)
    assert not status.any() and sad.dtype == np.uint32 and sad.shape == (len(pairs), ncy, ncx, 2 * R + 1, 2 * R + 1)
    for k, (p, m) in enumerate(pairs):
        assert np.array_equal(sad[k], fieldref.surfaces(p, m, R)), (R, w, h, k)
    return sad


@pytest.mark.parametrize("R", RADII)
def test_kernel_against_numpy_at_the_definitions_sizes(R):
    for w, h in field_sizes(R):
        rs = np.random.RandomState(1000 * R + w)
        sad = check(field_contents(w, h, rs), R)
        assert not sad[1][..., R, R].any() and (sad[2] == sad[2][:, :, :1, :1]).all() and (sad[3] == 255 * C * C).all()


def test_every_radius():
    """each radius is a kernel of its own: two cells across with odd margins"""
    rs = np.random.RandomState(56)
    for R in range(1, 9):
        w, h = 2 * C + 2 * R + 5, C + 2 * R + 3
        check([(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)) for _ in range(2)], R)


@pytest.mark.parametrize("R", (2, 4, 8))
def test_planted_displacements(R):
    frame, model, moves = planted(R)
    sad = check([(frame, model)], R)
    rec = fieldref.records(sad[0], R)
    assert [[tuple(rec[cy, cx, :2]) for cx in range(2)] for cy in range(2)] == moves and all(fieldref.rated(r) for r in rec.reshape(-1, 5))


def test_every_residue_of_the_offsets():
    """the frame at every offset mod 16 against the model at every offset mod 16: 256 jobs of one size, all the same surface;
    an odd width, so the rows themselves begin at every residue"""
    R, w, h = 4, C + 2 * 4 + 3, C + 2 * 4 + 1
    rs = np.random.RandomState(9)
    p, m = rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)
    n, step = w * h, (w * h + 31) // 16 * 16
    fr, mu = np.full(16 * step + 16, 0xEE, np.uint8), np.full(16 * step + 16, 0x11, np.uint8)
    for r in range(16):
        fr[r * step + r:r * step + r + n], mu[r * step + r:r * step + r + n] = p.reshape(-1), m.reshape(-1)
    jobs = [(a * step + a, b * step + b) for a in range(16) for b in range(16)]
    status, sad = hip.frame_shift_cells(torch.from_numpy(fr).to(DEV), torch.from_numpy(mu).to(DEV), jobs, w, h, R)
    want = fieldref.surfaces(p, m, R)
    assert not status.any() and all(np.array_equal(s, want) for s in sad)
    # ... and the buffers themselves at an odd address, their sizes exact: the last frame ends where the buffer ends
    d_fr, d_mu = torch.from_numpy(np.concatenate([[0, 0, 0], p.reshape(-1)]).astype(np.uint8)).to(DEV), torch.from_numpy(
        np.concatenate([[0], m.reshape(-1)]).astype(np.uint8)).to(DEV)
    status, sad = hip.frame_shift_cells(d_fr[3:], d_mu[1:], [(0, 0)], w, h, R)
    assert not status.any() and np.array_equal(sad[0], want)


def test_the_order_of_the_jobs_does_not_matter():
    R, w, h = 4, 2 * C + 2 * 4 + 5, C + 2 * 4 + 3
    rs = np.random.RandomState(31)
    pairs = [(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)) for _ in range(5)]
    fr, mu, jobs = pack(pairs, align=16)
    _, sad = hip.frame_shift_cells(fr, mu, jobs, w, h, R)
    status, back = hip.frame_shift_cells(fr, mu, jobs[::-1], w, h, R)
    assert not status.any() and np.array_equal(back[::-1], sad)
    for k, job in enumerate(jobs):
        _, one = hip.frame_shift_cells(fr, mu, [job], w, h, R)
        assert np.array_equal(one[0], sad[k])
    for k, (p, m) in enumerate(pairs):
        assert np.array_equal(sad[k], fieldref.surfaces(p, m, R))


def test_seventy_thousand_jobs():
    """more jobs than a grid dimension holds (65,535): blocks take several jobs each.  The jobs alias three frames and three
    models of one cell each, every pairing"""
    R, n, s = 1, 70000, C + 2
    rs = np.random.RandomState(3)
    p, m = rs.randint(0, 256, (3, s, s)).astype(np.uint8), rs.randint(0, 256, (3, s, s)).astype(np.uint8)
    k = np.arange(n)
    jobs = np.stack([(k % 3) * s * s, (k // 3 % 3) * s * s], axis=1)
    status, sad = hip.frame_shift_cells(torch.from_numpy(p).to(DEV), torch.from_numpy(m).to(DEV), jobs, s, s, R)
    want = np.array([[fieldref.surfaces(p[a], m[b], R) for b in range(3)] for a in range(3)])
    assert not status.any() and np.array_equal(sad, want[k % 3, k // 3 % 3])


def test_jobs_past_their_buffers_and_canaries():
    """job 1 runs past frames_bytes by one byte, job 3 past model_bytes, jobs 5 and 6 have an offset beyond any buffer: status
    set, surface zero, nothing of them read; their neighbours are intact.  status and sad lie inside larger tensors whose
    other words must keep their values."""
    R, w, h = 4, 2 * C + 2 * 4 + 2, C + 2 * 4 + 1
    n, D = w * h, 2 * R + 1
    words = 2 * D * D  # two cells
    rs = np.random.RandomState(41)
    pairs = [(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)) for _ in range(4)]
    fr, mu, jobs = pack(pairs, align=16)
    end = 4 * ((n + 15) // 16 * 16)
    jobs = [jobs[0], (end - n + 1, 0), jobs[1], (0, end - n + 1), jobs[2], (1 << 40, 0), (0, (1 << 64) - 1), jobs[3]]
    nj = len(jobs)
    status_all = torch.full((nj + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    sad_all = torch.full((nj * words + 9,), 0x01234567, dtype=torch.int32, device=DEV)
    status, sad = hip.frame_shift_cells(fr, mu, jobs, w, h, R, frames_bytes=end, model_bytes=end, status=status_all[4:4 + nj],
                                        sad=sad_all[5:5 + nj * words])  # (an odd word: sad need only be 4-byte aligned)
    assert list(status) == [0, fieldref.E_RANGE, 0, fieldref.E_RANGE, 0, fieldref.E_RANGE, fieldref.E_RANGE, 0]
    for k, pair in zip((0, 2, 4, 7), pairs):
        assert np.array_equal(sad[k], fieldref.surfaces(pair[0], pair[1], R)), k
    assert not sad[[1, 3, 5, 6]].any()
    st, sd = status_all.cpu().numpy(), sad_all.cpu().numpy()
    assert (st[:4] == 0x5A5A5A5A).all() and (st[4 + nj:] == 0x5A5A5A5A).all()
    assert (sd[:5] == 0x01234567).all() and (sd[5 + nj * words:] == 0x01234567).all()
    # the same list one byte more generous: jobs 1 and 3 now end exactly where their buffers end, and are read
    fr2, mu2 = torch.cat([fr[:end], fr[:1]]), torch.cat([mu[:end], mu[:1]])
    status, sad = hip.frame_shift_cells(fr2, mu2, jobs[:4], w, h, R)
    assert not status.any()
    a, b = fr2.cpu().numpy(), mu2.cpu().numpy()
    assert np.array_equal(sad[1], fieldref.surfaces(a[end - n + 1:end + 1].reshape(h, w), b[:n].reshape(h, w), R))
    assert np.array_equal(sad[3], fieldref.surfaces(a[:n].reshape(h, w), b[end - n + 1:end + 1].reshape(h, w), R))


def test_a_full_size_frame_at_the_largest_radius():
    """1680 x 1050 at R = 8: 13 x 8 cells of 289 words each"""
    rs = np.random.RandomState(77)
    w, h, R = 1680, 1050, 8
    sad = check([(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8))], R)
    assert sad.shape == (1, 8, 13, 17, 17)


def test_every_cell_is_the_frame_search_of_its_crops():
    """the existing kernel, abub_frame_shift_dev, run on each cell's (128 + 2 R)^2 crops as frames of their own: the cell is
    the crop's interior, so its surface is the crop's"""
    R, w, h = 4, 2 * C + 2 * 4 + 1, 2 * C + 2 * 4 + 2
    rs = np.random.RandomState(13)
    p, m = rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)
    fr, mu, jobs = pack([(p, m)])
    _, sad = hip.frame_shift_cells(fr, mu, jobs, w, h, R)
    cells = [(cx, cy) for cy in range(2) for cx in range(2)]
    crops = [(fieldref.crop(p, w, h, R, cx, cy), fieldref.crop(m, w, h, R, cx, cy)) for cx, cy in cells]
    fr, mu, jobs = pack(crops)
    status, whole = hip.frame_shift(fr, mu, jobs, C + 2 * R, C + 2 * R, R)
    assert not status.any()
    for k, (cx, cy) in enumerate(cells):
        assert np.array_equal(whole[k], sad[0, cy, cx].astype(np.uint64)), (cx, cy)
