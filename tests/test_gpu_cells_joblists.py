"""The four per-cell entries (abub_frame_shift_cells_dev, abub_frame_light_cells_dev, abub_frame_focus_cells_dev,
abub_frame_noise_cells_dev) on a job list in which a block takes a refused job and an accepted one, one after the other:
65,540 jobs of one cell, so that with the grid's 65,535 rows the blocks y = 0 .. 4 take the jobs y and y + 65,535, as
(refused, ok), (ok, refused), (refused, refused), (ok, ok) and (ok, ok on another frame).  Every other job is accepted; the
jobs alias three frames, as the frame and as the model (for the noise as the reference too).  A refused job runs one byte
past the frames; one of the noise's has its reference there instead.  status is E_RANGE on exactly the refused jobs, their
records are zero, every other record is the numpy definition's bit for bit, and the words round status and rec keep their
values."""
import numpy as np
import pytest
import torch

import fieldref
import focusref
import lightref
import noiseref
from autobub3hs_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = fieldref.CELL
ROWS = 65535  # of a grid
NJ = ROWS + 5
REFUSED = (0, 2, ROWS + 1, ROWS + 2)
R = 2

# entry -> (the frame's side: one cell and its ring, offsets of a job, the call, the definition of a record from a job's frames)
ENTRIES = {
    "field": (C + 2 * R, 2, lambda d, jobs, s, status, out: hip.frame_shift_cells(d, d, jobs, s, s, R, status=status, sad=out),
              lambda p, m: fieldref.surfaces(p, m, R)),
    "light": (C, 2, lambda d, jobs, s, status, out: hip.frame_light_cells(d, d, jobs, s, s, 0, 0, 1, 1, status=status, rec=out),
              lambda p, m: lightref.records(p, m, 0, 0, 1, 1)),
    "focus": (C + 2, 2, lambda d, jobs, s, status, out: hip.frame_focus_cells(d, d, jobs, s, s, 1, 1, 1, 1, status=status, rec=out),
              lambda p, m: focusref.records(p, m, 1, 1, 1, 1)),
    "noise": (C, 3, lambda d, jobs, s, status, out: hip.frame_noise_cells(d, d, jobs, s, s, 0, 0, 1, 1, status=status, rec=out),
              lambda p, r, m: noiseref.records(p, r, m, 0, 0, 1, 1)),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_block_takes_refused_and_accepted_jobs_in_turn(entry):
    side, nof, call, define = ENTRIES[entry]
    assert fieldref.grid(C + 2 * R, C + 2 * R, R) == (1, 1, R, R)
    n = side * side
    f = np.random.RandomState(600 + side).randint(0, 256, (3, side, side)).astype(np.uint8)
    f[0, :9] = 0
    f[1, -9:] = 255
    k = np.arange(NJ)
    which = np.stack([k // 3 ** q % 3 for q in range(nof)], axis=1)  # the frame behind each offset of job k
    which[ROWS + 4, 0] = (which[4, 0] + 1) % 3
    jobs = which * n
    past = 2 * n + 1  # a frame from here on ends one byte behind the buffer
    for j in REFUSED:
        jobs[j, 1 if entry == "noise" and j == ROWS + 2 else 0] = past
    ok = np.ones(NJ, bool)
    ok[list(REFUSED)] = False
    # a block's two jobs: (refused, ok), (ok, refused), (refused, refused), (ok, ok), (ok, ok on another frame)
    assert [(bool(ok[y]), bool(ok[y + ROWS])) for y in range(5)] == [(False, True), (True, False), (False, False), (True, True), (True, True)]
    assert which[4, 0] != which[ROWS + 4, 0]
    want = np.array([define(*(f[a] for a in abc)) for abc in np.ndindex(*(3,) * nof)])
    words = want[0].size
    want = want.reshape(*(3,) * nof, words).astype(np.int64)
    d = torch.from_numpy(f).to(DEV)
    status_all = torch.full((NJ + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    rec_all = torch.full((NJ * words + 9,), 0x01234567, dtype=torch.int32, device=DEV)
    status, rec = call(d, jobs, side, status_all[4:4 + NJ], rec_all[5:5 + NJ * words])
    assert np.array_equal(status, np.where(ok, 0, fieldref.E_RANGE))
    rec = rec.reshape(NJ, words).astype(np.int64)
    assert not rec[~ok].any()
    assert np.array_equal(rec[ok], want[tuple(which[ok].T)])
    st, rc = status_all.cpu().numpy(), rec_all.cpu().numpy()
    assert (st[:4] == 0x5A5A5A5A).all() and (st[4 + NJ:] == 0x5A5A5A5A).all()
    assert (rc[:5] == 0x01234567).all() and (rc[5 + NJ * words:] == 0x01234567).all()
