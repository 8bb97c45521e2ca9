"""The float stage of the bellows matcher (abub_match_best_batch_dev: k_match_tnorm, k_match_norm, k_match_first,
k_match_sub) against the numpy definition (tests/matchref.py) and the host's bestMatchFromTerms, bit for bit: the three
branches of the normalisation, exact ties across waves and blocks, maxima on corners and edges, tiny planes, several jobs
with different ranges in one call, and a scratch full of garbage.  Every call has best_xy and the scratch inside larger
tensors filled with 0x5A, whose bytes outside what the call owns must keep their value."""
import numpy as np
import pytest

import matchref
from matchref import match_geometry, same_xy

from autobub3hs_amd import _lib, host

SCENES = matchref.scenes()
PAD = 0x5A


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


class Arena:
    """best_xy and the scratch of one shape, each inside a larger tensor of 0x5A bytes"""

    def __init__(self, W, H, tw, th, njobs, scratch_bytes=None):
        import torch

        self.njobs = njobs
        self.need = _lib.lib().abub_match_best_scratch_bytes(W, H, tw, th, njobs) if scratch_bytes is None else scratch_bytes
        assert self.need > 0
        self.big = torch.full((self.need + 1024,), PAD, dtype=torch.uint8, device="cuda:0")
        self.off = (-self.big.data_ptr()) % 256 + 256
        self.scratch = self.big[self.off:self.off + self.need]
        assert self.scratch.data_ptr() % 256 == 0
        self.big_xy = torch.full(((2 * njobs + 16) * 4,), PAD, dtype=torch.uint8, device="cuda:0").view(torch.float32)
        self.xy = self.big_xy[8:8 + 2 * njobs]

    def check_outside(self):
        import torch

        torch.cuda.synchronize()
        b = self.big
        assert bool((b[:self.off] == PAD).all()) and bool((b[self.off + self.need:] == PAD).all()), "scratch overrun"
        w = self.big_xy.view(torch.int32)
        assert bool((w[:8] == 0x5A5A5A5A).all()) and bool((w[8 + 2 * self.njobs:] == 0x5A5A5A5A).all()), "best_xy overrun"


def device_best(frames, idx, tmpl, arena=None):
    import torch

    from autobub3hs_amd import hip

    frames = np.ascontiguousarray(frames)
    assert 0 <= min(idx) and max(idx) < len(frames)  # every index stays inside the slab
    H, W = frames.shape[1:]
    th, tw = tmpl.shape
    if arena is None:
        arena = Arena(W, H, tw, th, len(idx))
    out = hip.match_best(torch.from_numpy(frames).to("cuda:0"), torch.tensor(idx, dtype=torch.int32, device="cuda:0"),
                         torch.from_numpy(tmpl).to("cuda:0"), scratch=arena.scratch, out=arena.xy)
    arena.check_outside()
    return out.cpu().numpy().reshape(len(idx), 2)


def reference_best(img, tmpl):
    """the numpy definition, checked against the host's bestMatchFromTerms on the same terms"""
    num, w2 = matchref.terms(img, tmpl)
    xy, idx, _ = matchref.best(matchref.plane(num, w2, tmpl)[0])
    assert same_xy(xy, host.best_match(num, w2, tmpl))
    return xy


@pytest.mark.gpu
@pytest.mark.parametrize("name,img,tmpl,what", SCENES, ids=[s[0] for s in SCENES])
def test_scene_equals_the_definition(name, img, tmpl, what):
    """One job per scene (the conditions each scene meets are asserted in test_match_ref.py), then the scene among others."""
    want = reference_best(img, tmpl)
    if "nan" in what:
        assert bool(np.isnan(want).all()) == what["nan"]
    got = device_best(img[None], [0], tmpl)
    assert same_xy(got[0], want), (name, got[0], want)
    other = np.random.RandomState(len(name)).randint(0, 256, img.shape).astype(np.uint8)
    got = device_best(np.stack([other, img, other]), [1, 2, 1], tmpl)
    assert same_xy(got[0], want) and same_xy(got[2], want), (name, got, want)
    assert same_xy(got[1], reference_best(other, tmpl)), (name, got[1])


@pytest.mark.gpu
def test_several_jobs_with_different_ranges_in_one_call():
    """Random, tiled, flat and black-quarter frames as jobs [0, 1, 2, 3, 1, 0], the same list reversed, and one job per
    call: minKey / maxKey / best are kept per job, so every job's answer is the same on all three routes."""
    W, H, tw, th = 64, 48, 16, 12
    til, tmpl = matchref.tiled(W, H, tw, th)
    frames = np.stack([np.random.RandomState(71).randint(0, 256, (H, W)).astype(np.uint8), til, np.full((H, W), 77, np.uint8),
                       matchref.black_quarter(72, W, H)])
    want = [reference_best(f, tmpl) for f in frames]
    assert np.isnan(want[2]).all() and not np.isnan(np.concatenate([want[0], want[1], want[3]])).any()
    assert len({tuple(w.view(np.uint32)) for w in want}) == 4
    order = [0, 1, 2, 3, 1, 0]
    fwd = device_best(frames, order, tmpl)
    rev = device_best(frames, order[::-1], tmpl)
    for k, f in enumerate(order):
        single = device_best(frames, [f], tmpl)[0]
        assert same_xy(fwd[k], want[f]), (k, f, fwd[k], want[f])
        assert same_xy(rev[len(order) - 1 - k], want[f]), (k, f)
        assert same_xy(single, want[f]), (k, f, single)


@pytest.mark.gpu
def test_garbage_scratch_reused_across_split_and_plain_shapes():
    """One scratch full of 0x5A, then of the other shape's leftovers: the split path (whose atomics add into num) and the
    plain path give the same answers on every visit."""
    import torch

    A = (64, 200, 8, 130, 2)  # nsplit 4
    B = (64, 200, 8, 20, 2)   # nsplit 1
    assert match_geometry(*A)[0] == 4 and match_geometry(*B)[0] == 1
    rng = np.random.RandomState(81)
    frames = rng.randint(0, 256, (3, 200, 64)).astype(np.uint8)
    tA = frames[1, 30:160, 20:28].copy()
    tB = frames[2, 100:120, 50:58].copy()
    idx = [2, 1]
    need = max(_lib.lib().abub_match_best_scratch_bytes(*s) for s in (A, B))
    arena = Arena(*A, scratch_bytes=need)
    want = {"A": [reference_best(frames[f], tA) for f in idx], "B": [reference_best(frames[f], tB) for f in idx]}
    for visit in range(2):
        for key, t in (("A", tA), ("B", tB)):
            got = device_best(frames, idx, t, arena)
            for k in range(2):
                assert same_xy(got[k], want[key][k]), (visit, key, k, got[k], want[key][k])
    assert bool((arena.scratch != PAD).any())
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_misaligned_scratch_refused():
    """A scratch of the right size, 8 bytes off a 256-byte boundary: ABUB_E_INVALID, nothing written."""
    import torch

    W, H, tw, th, n = 40, 30, 6, 5, 2
    arena = Arena(W, H, tw, th, n)
    frames = torch.randint(0, 256, (1, H, W), dtype=torch.uint8, device="cuda:0")
    tmpl = torch.randint(0, 256, (th, tw), dtype=torch.uint8, device="cuda:0")
    fidx = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    off = arena.scratch[8:]  # the arena's pad behind the scratch keeps all of it inside the tensor
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    rc = L.abub_match_best_batch_dev(frames.data_ptr(), W, H, fidx.data_ptr(), n, tmpl.data_ptr(), tw, th, arena.xy.data_ptr(),
                                     off.data_ptr(), arena.need, st)
    torch.cuda.synchronize()
    assert rc == -1 and b"bad arguments" in L.abub_last_error()
    assert bool((arena.big == PAD).all()) and bool((arena.big_xy.view(torch.int32) == 0x5A5A5A5A).all())
    rc = L.abub_match_best_batch_dev(frames.data_ptr(), W, H, fidx.data_ptr(), n, tmpl.data_ptr(), tw, th, arena.xy.data_ptr(),
                                     arena.scratch.data_ptr(), arena.need, st)
    torch.cuda.synchronize()
    assert rc == 0
    arena.check_outside()
    assert same_xy(arena.xy.cpu().numpy()[:2], reference_best(frames[0].cpu().numpy(), tmpl.cpu().numpy()))
