"""K1 training (Trainer::CalculateMeanSigmaImageVector) restated in numpy float32, three mutants of it, and the pixels
designed to tell them apart.  No GPU, no oracle: this module is the definition the tests of K1 are counted with.

The recurrence, per pixel, over the frames in their given order (all arithmetic float32, one rounding per operation):

    delta = x - mean;  mean = mean + delta / (k + 1);  m2 = m2 + delta * (x - mean)
    sd = sqrt(m2 / (N - 1));  sigma = (int)sd, 0 where sd is NaN (N = 1);  mu = (int)mean

Bit parity with it rests on three things a build can lose without any random image noticing: the product and the sum
of the m2 update are rounded separately (no fused multiply-add), the divide is a correctly rounded divide (not a
multiplication by a rounded reciprocal), and divide and sqrt are correctly rounded at all.  The mutants make each of
those mistakes on purpose:

    "contract"  m2 + delta * (x - mean) with one rounding
    "recip"     delta * (1 / (k + 1))
    "low"       sd one float below the correctly rounded one (what a sqrt or divide that lands one ulp low gives)

designed() builds pixels whose exact standard deviation is an integer, where a float that lands just below changes
the truncated byte."""
import numpy as np

MODES = ("exact", "contract", "recip", "low")
DESIGNED_SEED = 20240607
ORDERINGS = 8  # orderings (and bases) per (N, n1, d)


def welford(st, mode="exact"):
    """st: u8 [N, P] or [N, H, W] -> (mu, sigma) u8 of shape st.shape[1:]."""
    assert mode in MODES, mode
    st = np.asarray(st)
    assert st.dtype == np.uint8 and st.ndim in (2, 3) and st.shape[0] >= 1
    N, shape = st.shape[0], st.shape[1:]
    f32 = np.float32
    mean = np.zeros(shape, f32)
    m2 = np.zeros(shape, f32)
    for k in range(N):
        x = st[k].astype(f32)
        d = x - mean
        if mode == "recip":
            mean = mean + d * (f32(1) / f32(k + 1))
        else:
            mean = mean + d / f32(k + 1)
        if mode == "contract":
            # the product of two float32 is exact in float64
            m2 = (m2.astype(np.float64) + d.astype(np.float64) * (x - mean).astype(np.float64)).astype(f32)
        else:
            m2 = m2 + d * (x - mean)
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(m2 / f32(N - 1))
    assert mean.dtype == f32 and m2.dtype == f32 and sd.dtype == f32
    if mode == "low":
        sd = np.nextafter(sd, f32(0))
    nan = np.isnan(sd)  # N = 1: 0 / 0
    sigma = np.where(nan, f32(0), sd).astype(np.int32).astype(np.uint8)
    return mean.astype(np.int32).astype(np.uint8), sigma


def _isqrt_exact(v):
    r = int(round(v ** 0.5))
    for c in (r - 1, r, r + 1):
        if c >= 0 and c * c == v:
            return c
    return None


def triples():
    """Every (N, n1, d, sd) with 3 <= N <= 40, 1 <= n1 < N, 1 <= d <= 255 for which the sample variance of N - n1
    values a and n1 values a + d, n1 (N - n1) d^2 / (N (N - 1)), is a non-zero perfect square sd^2."""
    out = []
    for N in range(3, 41):
        for n1 in range(1, N):
            for d in range(1, 256):
                num, den = n1 * (N - n1) * d * d, N * (N - 1)
                if num % den:
                    continue
                sd = _isqrt_exact(num // den)
                if sd:
                    out.append((N, n1, d, sd))
    return out


def designed(seed=DESIGNED_SEED):
    """{N: u8 [N, n_pixels]}: per triple ORDERINGS pixels, each with its own base a in [0, 255 - d] and its own
    order of the N - n1 values a and n1 values a + d (the recurrence is not order independent)."""
    rs = np.random.RandomState(seed)
    cols = {}
    for N, n1, d, _ in triples():
        for _ in range(ORDERINGS):
            a = rs.randint(0, 256 - d)
            col = np.full(N, a, np.uint8)
            col[:n1] = a + d
            cols.setdefault(N, []).append(col[rs.permutation(N)])
    return {N: np.ascontiguousarray(np.stack(c, axis=1)) for N, c in sorted(cols.items())}


def differ(st, mode):
    """Number of pixels of st whose (mu, sigma) under the mutant `mode` is not that of the exact recurrence."""
    mu, sg = welford(st)
    mu_m, sg_m = welford(st, mode)
    return int(np.count_nonzero((mu != mu_m) | (sg != sg_m)))


def noisy_frames(rs, n, H, W, amp=3):
    """Base plus small noise: the realistic training set (small sigma, truncation boundaries)."""
    base = rs.randint(30, 200, (H, W))
    return np.clip(base[None] + rs.randint(-amp, amp + 1, (n, H, W)), 0, 255).astype(np.uint8)


def as_plane(group, H, W):
    """The first H * W pixels of a designed group [N, n] as frames [N, H, W]."""
    assert group.shape[1] >= H * W
    return np.ascontiguousarray(group[:, :H * W]).reshape(group.shape[0], H, W)
