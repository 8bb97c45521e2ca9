"""The bellows template matcher, defined in numpy: the exact integer terms of cv::matchTemplate(CV_TM_CCORR_NORMED), the
CV_32F correlation plane and the best match with its 3x3 centre of mass -- a line-by-line restatement of
bestMatchFromTerms (host/hostlogic.cpp), in the host's order and precision -- and the scenes the matcher's tests share."""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)
DIV, CLAMP, ZERO = 0, 1, 2  # the branch a placement takes in plane()
TH_MAX = 66051  # tallest template the matcher takes: 66051 * 255 * 255 < 2^32 <= 66052 * 255 * 255


def match_geometry(W, H, tw, th, njobs):
    """(nsplit, template rows per workgroup, flush interval in image rows) of k_match_num (match_geom, abub_match.hip)"""
    rw, rh = W - tw + 1, H - th + 1
    ybl = (rh + 31) // 32
    base = ((rw + 255) // 256) * ybl * njobs
    nsplit = 1 if base >= 1024 else min((1024 + base - 1) // base, max(1, th // 32))
    rsplit = (th + nsplit - 1) // nsplit
    return (th + rsplit - 1) // rsplit, rsplit, 0xffffffff // (65025 * tw)


def match_chunks(tw):
    """(nc, rc): words per template row and template rows per LDS chunk of k_match_num (MTPL = 1024 entries)"""
    nc = (tw + 2) // 4 + 1
    return nc, max(1, 1024 // nc)


def same_xy(a, b):
    """Bit-identical float32 pairs; a flat plane has zero mass and gives NaN on every route (any NaN matches)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return all((np.isnan(u) and np.isnan(v)) or u.view(np.uint32) == v.view(np.uint32) for u, v in zip(a, b))


def terms(img, tmpl):
    """num = sum(T*I) and wsum2 = sum(I*I) per placement, exact, as u64 [H-th+1, W-tw+1]."""
    img, tmpl = np.asarray(img), np.asarray(tmpl)
    assert img.dtype == np.uint8 and tmpl.dtype == np.uint8 and img.ndim == 2 and tmpl.ndim == 2
    th, tw = tmpl.shape
    H, W = img.shape
    assert th <= H and tw <= W
    I = img.astype(np.int64)  # every sum stays below 2^63: 65025 * 4096 * 66051 < 1.8e16
    win = np.lib.stride_tricks.sliding_window_view(I, (th, tw))
    num = np.einsum("yxrc,rc->yx", win, tmpl.astype(np.int64))
    S = np.zeros((H + 1, W + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(I * I, axis=0), axis=1)
    w2 = S[th:, tw:] - S[:H - th + 1, tw:] - S[th:, :W - tw + 1] + S[:H - th + 1, :W - tw + 1]
    return num.astype(np.uint64), w2.astype(np.uint64)


def template_norm(tmpl):
    """sqrt(sdv^2 + mean^2) / sqrt(1/N) from the integer sums, in double (a Python float is a C double)."""
    t = np.asarray(tmpl).astype(np.uint64)
    N = float(t.size)
    s, q = float(int(t.sum())), float(int((t * t).sum()))
    inv_area = 1.0 / N
    mean = s * inv_area
    var = q * inv_area - mean * mean
    sdv = float(np.sqrt(np.float64(var if var > 0 else 0.0)))
    norm = float(np.sqrt(np.float64(sdv * sdv + mean * mean)))
    return norm / float(np.sqrt(np.float64(inv_area)))


def plane(num, wsum2, tmpl):
    """The CV_32F correlation plane and, per placement, the branch it took: DIV (v / t), CLAMP (t <= |v| < 1.125 t -> 1)
    or ZERO (a zero window, t = 0)."""
    num, wsum2 = np.asarray(num, np.uint64), np.asarray(wsum2, np.uint64)
    tn = np.float64(template_norm(tmpl))
    v = num.astype(np.float64).astype(np.float32).astype(np.float64)  # (double)(float)(double)num
    w2 = wsum2.astype(np.float64)
    lim = np.float64(np.float32(10) * np.float32(FLT_EPSILON)) * w2
    t = np.where(w2 <= np.minimum(0.5, lim), 0.0, np.sqrt(w2) * tn)
    branch = np.where(np.abs(v) < t, DIV, np.where(np.abs(v) < t * 1.125, CLAMP, ZERO)).astype(np.uint8)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(branch == DIV, v / t, np.where(branch == CLAMP, np.where(v > 0, 1.0, -1.0), 0.0))
    return r.astype(np.float32), branch


def best(res):
    """((x, y) as float32, winning raster index, normalised plane) of a correlation plane: normalize(NORM_MINMAX), the first
    maximum in raster order, and the 3x3 centre of mass around it (x offset outer, y offset inner, all in float32)."""
    res = np.asarray(res, np.float32)
    rh, rw = res.shape
    smin, smax = float(res.min()), float(res.max())
    scale = 1.0 / (smax - smin) if smax - smin > DBL_EPSILON else 0.0
    a, b = np.float32(scale), np.float32(0.0 - smin * scale)
    norm = res * a  # two float32 operations, each rounded
    norm = norm + b
    assert norm.dtype == np.float32
    idx = int(np.argmax(norm))  # the first maximum
    mx, my = idx % rw, idx // rw
    sx = sy = mass = np.float32(0)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            x, y = mx + i, my + j
            if x < 0 or y < 0 or x >= rw or y >= rh:
                continue
            pv = norm[y, x]
            sx = sx + np.float32(x) * pv
            sy = sy + np.float32(y) * pv
            mass = mass + pv
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.float32(np.float64(1.0) / np.float64(mass))
        xy = np.array([sx * inv, sy * inv], np.float32)
    return xy, idx, norm


def match(img, tmpl):
    """(xy, index, normalised plane, branches, correlation plane) of one frame and one template"""
    num, w2 = terms(img, tmpl)
    res, branch = plane(num, w2, tmpl)
    xy, idx, norm = best(res)
    return xy, idx, norm, branch, res


# ---- scenes of the float stage -------------------------------------------------------------------------------------------
# name -> (frame, template, expectation); the expectations are asserted from this reference alone in test_match_ref.py

def _rand(seed, H, W, lo=0, hi=256):
    return np.random.RandomState(seed).randint(lo, hi, (H, W)).astype(np.uint8)


def tiled(W, H, tw, th, spoiled=0, seed=21):
    """A frame tiled from its template (values 1..254); the first `spoiled` tiles in raster order are one grey level up."""
    tmpl = _rand(seed, th, tw, 1, 255)
    img = np.tile(tmpl, (H // th + 1, W // tw + 1))[:H, :W].copy()
    nx = (W - tw) // tw + 1  # whole tiles per row
    for k in range(spoiled):
        y, x = (k // nx) * th, (k % nx) * tw
        img[y:y + th, x:x + tw] += 1
    return img, tmpl


def tile_index(W, tw, th, k):
    """raster index, in the plane, of whole tile k of tiled()"""
    nx = (W - tw) // tw + 1
    return (k // nx) * th * (W - tw + 1) + (k % nx) * tw


def black_quarter(seed=31, W=70, H=52):
    img = _rand(seed, H, W, 1, 256)
    img[:H // 2, :W // 2] = 0
    return img


def pasted(seed=41, W=90, H=60, tw=12, th=9):
    """A random frame with its random template pasted unchanged at three places -> (frame, template, [(x, y)])"""
    img, tmpl = _rand(seed, H, W), _rand(seed + 1, th, tw)
    at = [(7, 3), (61, 20), (30, 47)]
    for x, y in at:
        img[y:y + th, x:x + tw] = tmpl
    return img, tmpl, at


BORDERS = ("nw", "n", "ne", "w", "e", "sw", "s", "se")


def border_cut(where, seed=51, W=61, H=47, tw=11, th=8):
    """The template cut from a corner or the middle of an edge of a random frame -> (frame, template, (mx, my))"""
    img = _rand(seed, H, W)
    rw, rh = W - tw + 1, H - th + 1
    mx = 0 if "w" in where else rw - 1 if "e" in where else rw // 2
    my = 0 if "n" in where else rh - 1 if "s" in where else rh // 2
    return img, img[my:my + th, mx:mx + tw].copy(), (mx, my)


def scenes():
    """[(name, frame, template, what)]: what is a dict of the conditions the scene is built to meet -- "nan": the result is
    NaN; "index": the winning raster index; "clamp" / "zero": at least that many placements in that branch; "ties": at
    least that many maxima of the normalised plane; "equal_at": placements (x, y) whose correlation is identical."""
    out = []
    img, tmpl, at = pasted()
    first = at[0][1] * (img.shape[1] - tmpl.shape[1] + 1) + at[0][0]
    out.append(("pasted", img, tmpl, {"equal_at": at, "index": first, "ties": 3}))  # the copies divide to exactly 1.0
    out.append(("saturated", np.full((30, 41), 255, np.uint8), np.full((7, 10), 255, np.uint8),
                {"clamp": 24 * 32, "nan": True}))
    out.append(("black_quarter", black_quarter(), _rand(32, 6, 9), {"zero": 101, "nan": False}))
    out.append(("zero_frame", np.zeros((33, 47), np.uint8), _rand(33, 5, 6), {"zero": 29 * 42, "nan": True}))
    out.append(("zero_template", _rand(34, 33, 47), np.zeros((5, 6), np.uint8), {"zero": 29 * 42, "nan": True}))
    out.append(("flat", np.full((33, 47), 77, np.uint8), _rand(35, 5, 6), {"nan": True}))
    for W, H, tw, th in ((64, 48, 16, 12), (130, 100, 50, 40)):
        for k in range(4):
            img, tmpl = tiled(W, H, tw, th, spoiled=k)
            what = {"index": tile_index(W, tw, th, k), "ties": 2 if k < 3 or W == 64 else 1}
            if W == 64:
                what["clamp"] = 16 - k  # here every unspoiled tile rounds into the clamp branch, next to DIV placements
            out.append(("tiled_%dx%d_spoiled%d" % (W, H, k), img, tmpl, what))
    for where in BORDERS:
        img, tmpl, (mx, my) = border_cut(where)
        out.append(("border_" + where, img, tmpl, {"index": my * (img.shape[1] - tmpl.shape[1] + 1) + mx}))
    out.append(("column_plane", _rand(61, 30, 9), _rand(62, 5, 9), {"shape": (26, 1)}))
    out.append(("row_plane", _rand(63, 6, 40), _rand(64, 6, 7), {"shape": (1, 34)}))
    out.append(("one_placement", _rand(65, 7, 9), _rand(66, 7, 9), {"shape": (1, 1), "nan": True}))
    out.append(("plane_3x5", _rand(67, 12, 13), _rand(68, 8, 11), {"shape": (5, 3)}))
    return out
