"""abub_frame_shift_dev (hip.frame_shift) bit for bit against the numpy restatement (tests/shiftref.py): the sizes and
contents of tests/test_shift_abi.py; widths around the dword, wave and tile edges; every residue mod 16 of the frame's and
the model's offset; the job list reversed and one job per call; 70,000 jobs (more than one grid can index); a frame whose
sums pass 2^32; jobs that run past their buffers; canaries round what the call writes."""
import numpy as np
import pytest
import torch

import shiftref
from autobub3hs_amd import hip
from test_shift_abi import RADII, interior, shift_contents, sizes

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
    status, sad = hip.frame_shift(fr, mu, jobs, w, h, R)
    assert not status.any()
    for k, (p, m) in enumerate(pairs):
        assert np.array_equal(sad[k], shiftref.surface(p, m, R)), (R, w, h, k)
    return sad


@pytest.mark.parametrize("R", RADII)
def test_kernel_against_numpy_at_the_definitions_sizes(R):
    for w, h in sizes(R):
        rs = np.random.RandomState(1000 * R + w)
        pairs = shift_contents(w, h, R, rs)
        sad = check(pairs, R)
        assert (sad[1] == 0).all() and (sad[2] == 255 * interior(w, h, R)).all() and (sad[3] == sad[2]).all()


def test_every_radius():
    """the radii between those of the other tests (each radius is a kernel of its own): a frame wider than a tile, so that
    both the path of a full tile and the masked one run, and a small one"""
    rs = np.random.RandomState(55)
    for R in range(1, 9):
        for w, h in ((300, 2 * R + 6), (2 * R + 3, 2 * R + 2)):
            check([(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)) for _ in range(2)], R)


@pytest.mark.parametrize("R", (2, 4))
def test_planted_displacements(R):
    w, h = 37, 29
    tex = np.random.RandomState(5 + R).randint(0, 256, (h + 2 * R, w + 2 * R)).astype(np.uint8)
    model = shiftref.displaced(tex, 0, 0, w, h, R)
    moves = [(dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    sad = check([(shiftref.displaced(tex, dx, dy, w, h, R), model) for dx, dy in moves], R)
    for k, (dx, dy) in enumerate(moves):
        assert sad[k][dy + R, dx + R] == 0 and shiftref.best(sad[k], R)["dx"] == dx and shiftref.best(sad[k], R)["dy"] == dy


@pytest.mark.parametrize("R", (1, 4))
def test_widths_at_the_dword_wave_and_tile_edges(R):
    """H = 2R + 3: an interior of three rows.  A lane owns four interior pixels and a tile is 256 of them wide, so with the
    halo of R the widths below put the interior's right edge on, before and behind a dword, a wave and a tile.  (A width below
    2R + 1 has no interior and is refused: those of the list are left out at R = 4.)  Then heights round the tile's 64 rows."""
    rs = np.random.RandomState(77 + R)
    rnd = lambda w, h: rs.randint(0, 256, (h, w)).astype(np.uint8)  # noqa: E731
    for w in (4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 256 + 2 * R - 1, 256 + 2 * R, 256 + 2 * R + 1, 512 + 2 * R + 3):
        if w >= 2 * R + 1:
            h = 2 * R + 3
            check([(rnd(w, h), rnd(w, h)), (rnd(w, h), rnd(w, h))], R)
    for h in (63, 64, 65, 64 + 2 * R, 64 + 2 * R + 1, 128 + 2 * R + 2):
        check([(rnd(21, h), rnd(21, h))], R)


def test_every_residue_of_the_offsets():
    """the frame at every offset mod 16 against the model at every offset mod 16: 256 jobs of one size, all the same surface"""
    R, w, h = 4, 67, 19
    rs = np.random.RandomState(9)
    p, m = rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)
    n, step = w * h, (w * h + 31) // 16 * 16
    fr, mu = np.full(16 * step + 16, 0xEE, np.uint8), np.full(16 * step + 16, 0x11, np.uint8)
    for r in range(16):
        fr[r * step + r:r * step + r + n], mu[r * step + r:r * step + r + n] = p.reshape(-1), m.reshape(-1)
    jobs = [(a * step + a, b * step + b) for a in range(16) for b in range(16)]
    status, sad = hip.frame_shift(torch.from_numpy(fr).to(DEV), torch.from_numpy(mu).to(DEV), jobs, w, h, R)
    want = shiftref.surface(p, m, R)
    assert not status.any() and all(np.array_equal(s, want) for s in sad)
    # ... and the buffers themselves at an odd address, their sizes exact: the last frame ends where the buffer ends
    d_fr, d_mu = torch.from_numpy(np.concatenate([[0, 0, 0], p.reshape(-1)]).astype(np.uint8)).to(DEV), torch.from_numpy(
        np.concatenate([[0], m.reshape(-1)]).astype(np.uint8)).to(DEV)
    status, sad = hip.frame_shift(d_fr[3:], d_mu[1:], [(0, 0)], w, h, R)
    assert not status.any() and np.array_equal(sad[0], want)


def test_the_order_of_the_jobs_does_not_matter():
    R, w, h = 4, 131, 21
    rs = np.random.RandomState(31)
    pairs = [(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)) for _ in range(7)]
    fr, mu, jobs = pack(pairs, align=16)
    _, sad = hip.frame_shift(fr, mu, jobs, w, h, R)
    status, back = hip.frame_shift(fr, mu, jobs[::-1], w, h, R)
    assert not status.any() and np.array_equal(back[::-1], sad)
    for k, job in enumerate(jobs):
        _, one = hip.frame_shift(fr, mu, [job], w, h, R)
        assert np.array_equal(one[0], sad[k])
    for k, (p, m) in enumerate(pairs):
        assert np.array_equal(sad[k], shiftref.surface(p, m, R))


def test_seventy_thousand_jobs():
    """more jobs than a grid dimension holds (65,535): blocks take several jobs each"""
    R, n = 1, 70000
    rs = np.random.RandomState(3)
    p, m = rs.randint(0, 256, (n, 3, 3)).astype(np.uint8), rs.randint(0, 256, (n, 3, 3)).astype(np.uint8)
    jobs = np.stack([np.arange(n) * 9, np.arange(n) * 9], axis=1)
    status, sad = hip.frame_shift(torch.from_numpy(p).to(DEV), torch.from_numpy(m).to(DEV), jobs, 3, 3, R)
    want = np.abs(p.astype(np.int64) - m[:, 1:2, 1:2].astype(np.int64)).astype(np.uint64)  # the interior is the one middle pixel
    assert not status.any() and np.array_equal(sad, want)


def test_a_frame_of_many_tiles_and_one_whose_sums_pass_2_to_the_32():
    """1680 x 1050: 7 x 17 tiles add into one surface.  4200 x 4200: 255 |I| no longer fits u32 (a block's partial sums
    do, the surface is u64)"""
    for w, h, radii in ((1680, 1050, (4, 8)), (4200, 4200, (4,))):
        fr, mu = torch.zeros(w * h, dtype=torch.uint8, device=DEV), torch.full((w * h,), 255, dtype=torch.uint8, device=DEV)
        for R in radii:
            status, sad = hip.frame_shift(fr, mu, [(0, 0)], w, h, R)
            assert not status.any() and (sad == 255 * interior(w, h, R)).all()
    assert 255 * interior(4200, 4200, 4) > 1 << 32


def test_jobs_past_their_buffers_and_canaries():
    """job 1 runs past frames_bytes by one byte, job 3 past model_bytes, job 5 has an offset beyond any buffer: status set,
    surface zero, nothing of them read; their neighbours are intact.  status and sad lie inside larger tensors whose other
    words must keep their values."""
    R, w, h = 4, 64, 20
    n, D = w * h, 2 * R + 1
    rs = np.random.RandomState(41)
    pairs = [(rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)) for _ in range(4)]
    fr, mu, jobs = pack(pairs, align=16)
    end = 4 * n
    jobs = [jobs[0], (end - n + 1, 0), jobs[1], (0, end - n + 1), jobs[2], (1 << 40, 0), (0, (1 << 64) - 1), jobs[3]]
    nj = len(jobs)
    status_all = torch.full((nj + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    sad_all = torch.full((nj * D * D + 8,), 0x0123456789ABCDEF, dtype=torch.int64, device=DEV)
    status, sad = hip.frame_shift(fr, mu, jobs, w, h, R, frames_bytes=end, model_bytes=end, status=status_all[4:4 + nj],
                                  sad=sad_all[4:4 + nj * D * D])
    assert list(status) == [0, shiftref.E_RANGE, 0, shiftref.E_RANGE, 0, shiftref.E_RANGE, shiftref.E_RANGE, 0]
    for k, pair in zip((0, 2, 4, 7), pairs):
        assert np.array_equal(sad[k], shiftref.surface(pair[0], pair[1], R)), k
    assert not sad[[1, 3, 5, 6]].any()
    st, sd = status_all.cpu().numpy(), sad_all.cpu().numpy()
    assert (st[:4] == 0x5A5A5A5A).all() and (st[4 + nj:] == 0x5A5A5A5A).all()
    assert (sd[:4] == 0x0123456789ABCDEF).all() and (sd[4 + nj * D * D:] == 0x0123456789ABCDEF).all()
    # the same list one byte more generous: jobs 1 and 3 now end exactly where their buffers end, and are read
    fr2, mu2 = torch.cat([fr[:end], fr[:1]]), torch.cat([mu[:end], mu[:1]])
    status, sad = hip.frame_shift(fr2, mu2, jobs[:4], w, h, R)
    assert not status.any()
    a, b = fr2.cpu().numpy(), mu2.cpu().numpy()
    assert np.array_equal(sad[1], shiftref.surface(a[end - n + 1:end + 1].reshape(h, w), b[:n].reshape(h, w), R))
    assert np.array_equal(sad[3], shiftref.surface(a[:n].reshape(h, w), b[end - n + 1:end + 1].reshape(h, w), R))
