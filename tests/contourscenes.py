"""K5 (abub_trace_contours_dev) test scenes: mask generators, the kept list of a set of frames as K4b leaves it, the launch
and compare helpers of test_gpu_contours.py, and a plain Python border follower that recounts the chain lengths of a frame
(what decides whether K5 may decline it).

Not collected by pytest.  Nothing here needs a GPU until launch() is called."""
import numpy as np

try:
    import torch
except ImportError:  # the generators and the recount work without it
    torch = None

DEV = "cuda:0"


def masks(rs):
    """the four random mask families of test_blobs_abi._masks (same draws for the same RandomState) and its two fixed ones"""
    out = []
    for _ in range(60):  # sparse noise
        H, W = rs.randint(1, 40), rs.randint(1, 40)
        out.append(rs.rand(H, W) < rs.choice([0.05, 0.2, 0.4, 0.6]))
    for _ in range(60):  # rings with components inside their holes, touching the edges and corners
        H, W = rs.randint(6, 40), rs.randint(6, 40)
        m = rs.rand(H, W) < 0.08
        for _ in range(rs.randint(1, 4)):
            h, w = rs.randint(3, 12), rs.randint(3, 12)
            y, x = rs.randint(-2, H - 1), rs.randint(-2, W - 1)
            y0, y1, x0, x1 = max(y, 0), min(y + h, H), max(x, 0), min(x + w, W)
            if y1 - y0 < 1 or x1 - x0 < 1:
                continue
            m[y0:y1, x0:x1] = True
            m[y0 + 1:y1 - 1, x0 + 1:x1 - 1] = False
            iy, ix = (y0 + y1) // 2, (x0 + x1) // 2
            m[iy, ix] = True  # a dot (or more) inside the hole
            if rs.rand() < 0.5 and iy + 1 < y1 - 1:
                m[iy + 1, ix] = True
        out.append(m)
    for _ in range(40):  # blobs of every size near the 10-pixel box limit
        H, W = rs.randint(5, 30), rs.randint(5, 30)
        m = np.zeros((H, W), bool)
        for _ in range(rs.randint(1, 8)):
            h, w = rs.randint(1, 6), rs.randint(1, 6)
            y, x = rs.randint(0, H), rs.randint(0, W)
            m[y:y + h, x:x + w] = rs.rand(min(h, H - y), min(w, W - x)) < 0.8
        out.append(m)
    for _ in range(40):  # one row, one column
        n = rs.randint(1, 80)
        m = rs.rand(n) < rs.choice([0.3, 0.7])
        out.append(m[None, :] if rs.rand() < 0.5 else m[:, None])
    out.append(np.ones((5, 5), bool))
    ring = np.ones((5, 5), bool)
    ring[1:4, 1:4] = False
    ring[2, 2] = True
    out.append(ring)  # the smallest enclosing ring
    return out


def place(m, H, W, corner):
    """mask m (cropped where it is larger than the frame) flush to the top-left (corner 0) or bottom-right corner of H x W"""
    m = m[:H, :W]
    f = np.zeros((H, W), bool)
    if corner == 0:
        f[:m.shape[0], :m.shape[1]] = m
    else:
        f[H - m.shape[0]:, W - m.shape[1]:] = m
    return f


def kept_list(frames):
    """-> (kept_off int64 [n+1], kept_idx int64): per frame its foreground's raster indices, increasing, as K4b leaves them"""
    offs, idx = [0], []
    for f in frames:
        i = np.flatnonzero(np.asarray(f).ravel())
        idx.append(i)
        offs.append(offs[-1] + len(i))
    return np.array(offs, np.int64), (np.concatenate(idx) if idx else np.zeros(0, np.int64))


def launch(frames, W, H, **kw):
    """hip.trace_contours on the kept list of `frames` -> dict of numpy arrays"""
    from autobub3hs_amd import hip

    offs, idx = kept_list(frames)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV)  # noqa: E731
    out = hip.trace_contours(t(offs), t(np.concatenate([idx, [0]])), W, H, in_cap=max(len(idx), 1), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def contours_of(out, s):
    """the contours of slot s as K5 wrote them -> list of int32 [npts, 2] (x, y)"""
    co, po = out["cont_off"].astype(np.int64), out["pt_off"].astype(np.int64)
    assert co[s + 1] - co[s] == out["ncont"][s]
    res, o = [], po[s]
    for n in out["cont_npts"][co[s]:co[s + 1]]:
        p = out["pts"][o:o + n].astype(np.int64) & 0xffffffff
        res.append(np.stack([p & 0xffff, p >> 16], axis=1).astype(np.int32))
        o += n
    assert o == po[s + 1]
    return res


def host_contours(frame):
    """the host route: ContourFinder::find on the frame's foreground pixels"""
    from autobub3hs_amd import host

    H, W = frame.shape
    idx = np.flatnonzero(np.asarray(frame).ravel()).astype(np.uint32)
    return host.contours_from_indices(idx, W, H) if len(idx) else []


def same(got, ref):
    """count, order and vertices"""
    return len(got) == len(ref) and all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, ref))


_DX = (1, 1, 0, -1, -1, -1, 0, 1)  # Freeman codes, y pointing down
_DY = (0, -1, -1, -1, 0, 1, 1, 1)


def chain_lengths(frame):
    """Suzuki-Abe outer border following with OpenCV's marks and scan rule (RETR_EXTERNAL), as the host does it -> the
    number of Freeman codes of every border traced, in discovery order (0: an isolated pixel)"""
    H, W = frame.shape
    img = np.zeros((H + 2, W + 2), np.int16)
    img[1:-1, 1:-1] = np.asarray(frame) != 0
    out = []
    for y in range(1, H + 1):
        row = img[y]
        if not row.any():
            continue
        lnbd, prev = 0, 0
        for x in range(1, W + 2):
            p = int(row[x])
            if p == prev:
                continue
            if prev == 0 and p == 1:
                if not row[lnbd] > 0:
                    out.append(_trace(img, y, x))
                    p = int(row[x])
            elif p == 0 and prev >= 1:
                if prev & -2:
                    lnbd = x - 1
            prev = p
            if prev & -2:
                lnbd = x
    return out


def _trace(img, y0, x0):
    s, found = 4, False
    for _ in range(7):
        s = (s - 1) & 7
        if img[y0 + _DY[s], x0 + _DX[s]] != 0:
            y1, x1 = y0 + _DY[s], x0 + _DX[s]
            found = True
            break
    if not found:
        img[y0, x0] = -126
        return 0
    y3, x3, n = y0, x0, 0
    while True:
        s_end = s
        while s < 15:
            s += 1
            y4, x4 = y3 + _DY[s & 7], x3 + _DX[s & 7]
            if img[y4, x4] != 0:
                break
        s &= 7
        if 0 <= s - 1 < s_end:
            img[y3, x3] = -126
        elif img[y3, x3] == 1:
            img[y3, x3] = 2
        n += 1
        if (y4, x4) == (y0, x0) and (y3, x3) == (y1, x1):
            return n
        y3, x3 = y4, x4
        s = (s + 4) & 7
