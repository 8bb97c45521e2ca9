"""The CPU oracle's K1 (orc_welford) against the numpy float32 definition of tests/trainref.py, and the conditions
under which the GPU tests of K1 (tests/test_gpu_train.py) can see a lost rounding at all.

The sensitivity counts are made with the numpy restatement alone, never with code under test: they say how many of the
designed pixels change their (mu, sigma) bytes when the recurrence is contracted to a fused multiply-add, when the
divide becomes a multiplication by a reciprocal, and when sd lands one float low.  A test on those pixels that passes
is then a statement about the build; on random images it would not be (a dozen random frames of a megapixel differ in
two pixels under contraction)."""
import numpy as np
import pytest

import trainref

# floors of the sensitivity counts over the whole designed set; if another seed falls below one, change the seed
FLOOR = {"contract": 200, "recip": 200, "low": 2000}


@pytest.fixture(scope="module")
def groups():
    return trainref.designed()


def same(oracle, st):
    """oracle.welford(st) == trainref.welford(st); st is [N, H, W]."""
    mu_r, sg_r = trainref.welford(st)
    mu, sg = oracle.welford(st)
    assert np.array_equal(mu, mu_r)
    assert np.array_equal(sg, sg_r)
    return mu, sg


def test_designed_set_is_what_it_says(groups):
    tr = trainref.triples()
    assert len(tr) == 1752 and sorted({t[0] for t in tr}) == [4, 9, 16, 25, 36]
    assert sorted(groups) == [4, 9, 16, 25, 36]
    assert sum(g.shape[1] for g in groups.values()) == 1752 * trainref.ORDERINGS == 14016
    for N, g in groups.items():
        assert g.dtype == np.uint8 and g.shape[0] == N and g.shape[1] % 8 == 0
        lo, hi = g.min(0).astype(int), g.max(0).astype(int)
        assert (hi > lo).all() and ((g == lo) | (g == hi)).all()  # two values per pixel
        n1, d = (g == hi).sum(0), hi - lo
        var = n1 * (N - n1) * d * d / (N * (N - 1))
        sd = np.rint(np.sqrt(var))
        assert (sd > 0).all() and np.array_equal(sd * sd, var)  # the exact variance is a perfect square
    again = trainref.designed()
    assert all(np.array_equal(groups[N], again[N]) for N in groups)  # fixed seed


def test_oracle_on_the_designed_set(oracle, groups):
    for N, g in groups.items():
        same(oracle, trainref.as_plane(g, 8, g.shape[1] // 8))


@pytest.mark.parametrize("mode", sorted(FLOOR))
def test_designed_set_is_sensitive(groups, mode):
    n = sum(trainref.differ(g, mode) for g in groups.values())
    print("pixels of the designed set that differ under %r: %d" % (mode, n))
    assert n >= FLOOR[mode], (mode, n)


def test_oracle_on_random_frames(oracle):
    st = np.random.RandomState(1234).randint(0, 256, (13, 9, 11)).astype(np.uint8)
    same(oracle, st)


def test_oracle_single_frame(oracle):
    st = np.random.RandomState(5).randint(0, 256, (1, 4, 5)).astype(np.uint8)
    mu, sg = same(oracle, st)
    assert np.array_equal(mu, st[0]) and not sg.any()


def test_oracle_two_frames(oracle):
    st = np.empty((2, 3, 4), np.uint8)
    st[0], st[1] = 0, 255
    mu, sg = same(oracle, st)
    assert (mu == 127).all() and (sg == 180).all()  # 255 / sqrt(2) = 180.31
    st[0] = 255
    mu, sg = same(oracle, st)
    assert (mu == 255).all() and not sg.any()


def test_oracle_long_run(oracle):
    same(oracle, trainref.noisy_frames(np.random.RandomState(300), 300, 16, 16, amp=3))


def test_restatement_modes():
    """'exact' is the default, [N, P] input gives [P] planes, an unknown mode is refused."""
    g = trainref.designed()[16]
    mu, sg = trainref.welford(g)
    assert all(np.array_equal(a, b) for a, b in zip(trainref.welford(g, "exact"), (mu, sg)))
    assert mu.shape == sg.shape == (g.shape[1],)
    with pytest.raises(AssertionError):
        trainref.welford(g, "fast")
