"""A numpy restatement of the DebugPeek planes and of the file set ("The peek planes"): what
abub_peek_planes_dev, the host route of host/peek.cpp and the reference's debug write-out all have to give."""
import numpy as np

# the six files of an accepted stack, in the order CalculateInitialBubbleParams writes them
SUFFIXES = ("000_AvgImage", "00_PreTrigFrame", "0_TrigFrame", "02_OvrThe6Sigma", "3_OtsuThresholded", "4_BubbleDetected")

E_SRC, E_DST, E_RECT = 1, 2, 3


def file_names(event, cam):
    return [f"ev{event}_cam{cam}_{s}.png" for s in SUFFIXES]


def thresholded(D, thr):
    """255 where D > thr, else 0 (the mask of foregroundKept(thr, -1))."""
    return np.where(np.asarray(D).astype(np.int64) > int(thr), 255, 0).astype(np.uint8)


def draw_rect(img, x, y, w, h):
    """cv::rectangle of host/cvlite.cpp, thickness 1, value 255, in place: written out pixel by pixel on purpose."""
    H, W = img.shape
    if w <= 0 or h <= 0:
        return
    x0, x1, y0, y1 = x, x + w - 1, y, y + h - 1
    for xx in range(max(x0, 0), min(x1, W - 1) + 1):
        if 0 <= y0 < H:
            img[y0, xx] = 255
        if 0 <= y1 < H:
            img[y1, xx] = 255
    for yy in range(max(y0, 0), min(y1, H - 1) + 1):
        if 0 <= x0 < W:
            img[yy, x0] = 255
        if 0 <= x1 < W:
            img[yy, x1] = 255


def presentation(frame, rects):
    out = np.array(frame, dtype=np.uint8, copy=True)
    for x, y, w, h in rects:
        draw_rect(out, int(x), int(y), int(w), int(h))
    return out


def item_status(item, P, diff_bytes, frames_bytes, out_bytes, nrects):
    """The status abub_peek_planes_dev gives an item (diff, frame, thr_out, pres_out, thr, rect_begin, rect_count)."""
    d, f, to, po, _, rb, rn = (int(v) for v in item)
    if d + P > diff_bytes or f + P > frames_bytes:
        return E_SRC
    if to % 16 or po % 16 or to + P > out_bytes or po + P > out_bytes or abs(to - po) < P:
        return E_DST
    if rb < 0 or rn < 0 or rb + rn > nrects:
        return E_RECT
    return 0


def planes(diff, frames, items, rects, W, H, out, diff_bytes=None, frames_bytes=None, out_bytes=None):
    """What the kernel leaves in `out` (a flat uint8 array; a copy is changed and returned) and in status[]."""
    diff, frames = np.asarray(diff).reshape(-1), np.asarray(frames).reshape(-1)
    out = np.array(out, dtype=np.uint8, copy=True).reshape(-1)
    rects = np.asarray(rects, dtype=np.int64).reshape(-1, 4)
    P = W * H
    db = len(diff) if diff_bytes is None else diff_bytes
    fb = len(frames) if frames_bytes is None else frames_bytes
    ob = len(out) if out_bytes is None else out_bytes
    status = np.zeros(len(items), np.int32)
    for k, it in enumerate(items):
        status[k] = item_status(it, P, db, fb, ob, len(rects))
        if status[k]:
            continue
        d, f, to, po, thr, rb, rn = (int(v) for v in it)
        out[to:to + P] = thresholded(diff[d:d + P], thr)
        out[po:po + P] = presentation(frames[f:f + P].reshape(H, W), rects[rb:rb + rn]).reshape(-1)
    return out, status
