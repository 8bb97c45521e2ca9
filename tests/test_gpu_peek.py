"""The DebugPeek planes on the GPU: abub_peek_planes_dev against the numpy restatement of tests/peekref.py, between
canaries (the whole output buffer is compared, so a byte written outside an item's two planes shows), at the smallest
shapes at which the kernel takes another path: widths below, at and above a 16-byte unit and a tile, one and several
rows, sources at every residue mod 16 (16-byte, 4-byte and single-byte loads, chosen independently for D and the frame),
thresholds at both ends with D holding thr and thr + 1 side by side, and every kind of rectangle cv::rectangle can be given."""
import numpy as np
import pytest
import torch

import peekref
from autobub3hs_amd import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = (4, 8, 60, 64, 68, 128, 1280)
HEIGHTS = (1, 2, 5, 33)
THRS = (0, 1, 254, 255)
# (residue of D, residue of the frame): every residue on both sides, and all nine pairs of load widths
RESIDUES = ([(k, k) for k in range(16)] + [(k, 15 - k) for k in range(16)]
            + [(0, 4), (0, 1), (4, 0), (8, 12), (4, 1), (1, 0), (1, 4), (3, 7)])


def rect_cases(W, H, rs):
    big = 2 ** 31 - 1
    return {
        "none": [],
        "1x1": [(W // 2, H // 2, 1, 1)],
        "1xh": [(W - 1, 0, 1, H)],
        "wx1": [(0, H - 1, W, 1)],
        "frame": [(0, 0, W, H)],
        "left": [(-3, H // 3, 6, 3)],
        "right": [(W - 2, 0, 5, 2)],
        "top": [(1, -2, 3, 4)],
        "bottom": [(0, H - 1, 3, 5)],
        "around": [(-1, -1, W + 2, H + 2)],  # crosses all four borders: no pixel of its outline is inside
        "corners": [(-2, -2, 4, 4), (W - 2, H - 2, 4, 4)],
        "outside": [(W, 0, 3, 3), (-5, -5, 3, 3), (0, H, 2, 2), (W + 10, H + 10, 5, 5), (big - 10, 0, 5, 5),
                    (-big - 1, -big - 1, big, big), (0, -big - 1, W, 7)],
        "empty": [(1, 0, 0, 3), (0, 0, -2, 2), (0, 0, 2, 0), (0, 0, 3, -1), (0, 0, 0, 0), (0, 0, -big, -big)],
        "overlap": [(0, 0, 3, 3), (1, 0, 3, 2)],
        "many": [(int(rs.randint(-8, W + 4)), int(rs.randint(-8, H + 4)), int(rs.randint(-1, W + 9)), int(rs.randint(-1, H + 9)))
                 for _ in range(300)],
    }


def d_plane(P, thr, rs):
    """random bytes with thr and thr + 1 (where they are bytes) side by side on most positions, the last ones included"""
    D = rs.randint(0, 256, P).astype(np.int64)
    near = rs.rand(P) < 0.6
    near[-min(P, 20):] = True
    D[near] = np.clip(thr + (np.arange(P)[near] & 1), 0, 255)
    return D.astype(np.uint8)


def garbage(n, seed):
    return ((np.arange(n, dtype=np.uint64) * 2654435761 + seed) >> 7).astype(np.uint8)


class Batch:
    """Items laid out in three host buffers: sources at the given residues mod 16, planes at multiples of 16 with gaps."""

    def __init__(self, W, H):
        self.W, self.H, self.P = W, H, W * H
        self.diff, self.frames, self.items, self.rects = [garbage(16, 1)], [garbage(16, 2)], [], []
        self.nd = self.nf = 16
        self.no = 16

    def _put(self, chunks, at, res, plane, seed):
        pad = (res - at) % 16 + 16 * (seed % 3)
        chunks.append(garbage(pad, seed))
        chunks.append(plane.reshape(-1))
        return at + pad, at + pad + self.P

    def add(self, D, frame, thr, rects, rd=0, rf=0):
        k = len(self.items)
        d_at, self.nd = self._put(self.diff, self.nd, rd, D, k)
        f_at, self.nf = self._put(self.frames, self.nf, rf, frame, k + 7)
        t_at = ((self.no + 15) & ~15) + 16 * (k % 3)
        p_at = ((t_at + self.P + 15) & ~15) + 16 * (k % 2)
        self.no = p_at + self.P + 5
        if k % 4 == 1:  # (which of the two planes comes first is the caller's choice)
            t_at, p_at = p_at, t_at
        self.items.append((d_at, f_at, t_at, p_at, thr, len(self.rects), len(rects)))
        self.rects += list(rects)

    def arrays(self):
        diff = np.concatenate(self.diff + [garbage(21, 3)])
        frames = np.concatenate(self.frames + [garbage(21, 4)])
        out = garbage((self.no + 15 & ~15) + 48, 5)
        return diff, frames, out

    def run(self, items=None, **sizes):
        diff, frames, out = self.arrays()
        items = self.items if items is None else items
        d_diff, d_frames, d_out = (torch.from_numpy(a).to(DEV) for a in (diff, frames, out))
        st = hip.peek_planes(d_diff, d_frames, items, self.rects, self.W, self.H, d_out, **sizes)
        torch.cuda.synchronize()
        assert np.array_equal(d_diff.cpu().numpy(), diff) and np.array_equal(d_frames.cpu().numpy(), frames)
        exp, est = peekref.planes(diff, frames, items, self.rects, self.W, self.H, out, **sizes)
        return d_out.cpu().numpy(), st, exp, est


@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", WIDTHS)
def test_planes_at_every_shape_residue_threshold_and_rectangle_kind(W, H):
    rs = np.random.RandomState(1000 * W + H)
    cases = rect_cases(W, H, rs)
    names = sorted(cases)
    b = Batch(W, H)
    used = set()
    for k, (rd, rf) in enumerate(RESIDUES):
        thr = THRS[k % 4] if k % 9 else int(rs.randint(2, 254))
        name = names[(k + k // len(names)) % len(names)]
        used.add(name)
        b.add(d_plane(W * H, thr, rs), rs.randint(0, 255, (H, W)).astype(np.uint8), thr, cases[name], rd, rf)
    assert used == set(names)
    assert {it[0] % 16 for it in b.items} == set(range(16)) == {it[1] % 16 for it in b.items}
    assert all(it[2] % 16 == 0 and it[3] % 16 == 0 for it in b.items)
    got, st, exp, est = b.run()
    assert not est.any() and np.array_equal(st, est)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (W, H, bad[:8], [k for k, it in enumerate(b.items) if any(it[o] <= bad[0] < it[o] + W * H for o in (2, 3))])


def test_every_threshold_against_every_byte():
    """The packed compare: all 256 byte values, in all four positions of a dword, against every threshold from below 0
    to above 255."""
    W, H = 272, 1
    D = np.concatenate([np.arange(256), [0, 255, 127, 128, 1, 254, 129, 126], np.arange(8) * 31]).astype(np.uint8)
    b = Batch(W, H)
    for k, thr in enumerate(list(range(-3, 259)) + [-2 ** 31, 2 ** 31 - 1, 1000, -1000]):
        b.add(np.roll(D, k), D[::-1].reshape(H, W), thr, [], rd=k % 3, rf=0)
    got, st, exp, est = b.run()
    assert not st.any() and np.array_equal(got, exp)


BAD = {
    "diff_past": (lambda it, s: (s["diff_bytes"] - s["P"] + 1,) + it[1:], peekref.E_SRC),
    "diff_far": (lambda it, s: (2 ** 63 + 5,) + it[1:], peekref.E_SRC),
    "frame_past": (lambda it, s: it[:1] + (s["frames_bytes"] - s["P"] + 1,) + it[2:], peekref.E_SRC),
    "thr_misaligned": (lambda it, s: it[:2] + (it[2] + 8,) + it[3:], peekref.E_DST),
    "pres_misaligned": (lambda it, s: it[:3] + (it[3] + 1,) + it[4:], peekref.E_DST),
    "thr_past": (lambda it, s: it[:2] + ((s["out_bytes"] - s["P"] + 16) & ~15,) + it[3:], peekref.E_DST),
    "pres_far": (lambda it, s: it[:3] + (2 ** 64 - 16,) + it[4:], peekref.E_DST),
    "planes_overlap": (lambda it, s: it[:3] + (it[2] + 16,) + it[4:], peekref.E_DST),
    "rect_begin_negative": (lambda it, s: it[:5] + (-1, 1), peekref.E_RECT),
    "rect_count_negative": (lambda it, s: it[:5] + (0, -1), peekref.E_RECT),
    "rects_past": (lambda it, s: it[:5] + (s["nrects"] - 1, 2), peekref.E_RECT),
    "rects_far": (lambda it, s: it[:5] + (2 ** 31 - 1, 2 ** 31 - 1), peekref.E_RECT),
}


@pytest.mark.parametrize("kind", sorted(BAD))
def test_bad_item_between_two_good_ones_is_refused_whole(kind):
    """The stated sizes are smaller than the tensors, so a descriptor that runs past them still points into memory the
    test owns; the refused item's planes keep their canary bytes and its neighbours are complete."""
    W, H = 68, 5
    rs = np.random.RandomState(7)
    b = Batch(W, H)
    for k in range(3):
        b.add(d_plane(W * H, 100, rs), rs.randint(0, 255, (H, W)).astype(np.uint8), 100, [(2 + k, 1, 9, 3), (-1, 0, 4, 4)], rd=k, rf=3 * k)
    diff, frames, out = b.arrays()
    sizes = dict(diff_bytes=len(diff) - 16, frames_bytes=len(frames) - 16, out_bytes=len(out) - 16)
    change, code = BAD[kind]
    items = list(b.items)
    items[1] = change(items[1], dict(sizes, P=W * H, nrects=len(b.rects)))
    got, st, exp, est = b.run(items, **sizes)
    assert list(est) == [0, code, 0] and list(st) == [0, code, 0]
    assert np.array_equal(got, exp)
    for o in (2, 3):  # (and the restatement did leave the refused item's planes alone, where they lie in the buffer)
        at = b.items[1][o]
        assert np.array_equal(exp[at:at + W * H], out[at:at + W * H])


def test_300_items_in_one_launch_equal_one_by_one():
    W, H = 68, 5
    rs = np.random.RandomState(11)
    cases = rect_cases(W, H, rs)
    names = sorted(n for n in cases if n != "many")
    b = Batch(W, H)
    for k in range(300):
        b.add(d_plane(W * H, k % 256, rs), rs.randint(0, 255, (H, W)).astype(np.uint8), k % 256, cases[names[k % len(names)]], rd=k % 16, rf=(5 * k) % 16)
    got, st, exp, est = b.run()
    assert not st.any() and np.array_equal(got, exp)
    diff, frames, out = b.arrays()
    d_diff, d_frames, d_out = (torch.from_numpy(a).to(DEV) for a in (diff, frames, out))
    for it in b.items:
        assert not hip.peek_planes(d_diff, d_frames, [it], b.rects, W, H, d_out).any()
    assert np.array_equal(d_out.cpu().numpy(), got)


def test_no_items_touch_nothing():
    out = torch.from_numpy(garbage(256, 9)).to(DEV)
    src = torch.zeros(64, dtype=torch.uint8, device=DEV)
    st = hip.peek_planes(src, src, [], [], 4, 4, out)
    assert st.size == 0 and np.array_equal(out.cpu().numpy(), garbage(256, 9))
