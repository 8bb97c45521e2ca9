"""Scenes, job lists and checks shared by the K2 / K3 scan tests (test_gpu_widths.py, test_gpu_joblists.py,
test_gpu_addressing.py, and the decision-boundary test of test_gpu_kernels.py).  The generators are numpy only; the
helpers that touch the device import torch and the package when they are called."""
import numpy as np

DEV = "cuda:0"
SENT = 0x5A5A5A5A  # canary word

# (dwords per lane, width): one full wave (64 lanes) and at least one partial wave per width class of the fast path
WIDTHS = [(1, 256), (1, 100), (2, 512), (2, 264), (3, 768), (3, 276), (4, 1024), (4, 560), (5, 1280), (5, 1100),
          (6, 1536), (6, 792), (7, 1792), (7, 1680), (7, 1400), (8, 2048), (8, 1088)]
PARTIAL_WIDTHS = [264, 276, 560, 1100, 792, 1400, 1088]  # the partial waves besides 100 and 1680

K2_DEFAULTS = (("bound", 1), ("chain", -1), ("budget", 1024), ("split", 1), ("list", 0), ("wg", -1), ("sync", -1),
               ("scanpf", -1), ("pf", 1), ("chunks", 0))
K3_DEFAULTS = (("scan", 1), ("list", 1), ("budget", 512), ("chunks", 0))

# (chain, split, list, wg, sync, scanpf) of the chained K2 scan
CHAIN_KNOBS = [(-1, 1, 0, -1, -1, -1), (2, 0, 1, 2, 1, 1), (4, 1, 1, 4, 2, 2), (4, 0, 0, 3, 0, 1)]


def restore_defaults():
    from autobub3hs_amd import hip

    for k, v in K2_DEFAULTS:
        hip.k2_set_option(k, v)
    for k, v in K3_DEFAULTS:
        hip.k3_set_option(k, v)


def set_chain_knobs(knobs):
    from autobub3hs_amd import hip

    for name, v in zip(("chain", "split", "list", "wg", "sync", "scanpf"), knobs):
        hip.k2_set_option(name, v)


def u32(t):
    return t.cpu().numpy().astype(np.uint32)


def check_list(pairs, count, imgs, thr, slots):
    """The fused list holds exactly the pixels of imgs[k] with value > thr[k] (a negative thr lists like 0), tagged
    slots[k], with their values; imgs / thr / slots are parallel."""
    n = int(count.item())
    assert n <= pairs.shape[0]
    pr = u32(pairs[:n])
    total = 0
    for img, t, slot in zip(imgs, thr, slots):
        sel = pr[(pr[:, 0] & 0xFFFFFF) == slot]
        exp = np.flatnonzero(img.ravel() > max(int(t), 0))
        order = np.argsort(sel[:, 1], kind="stable")
        assert np.array_equal(sel[order, 1], exp), slot
        assert np.array_equal((sel[order, 0] >> 24).astype(np.uint8), img.ravel()[exp]), slot
        total += len(exp)
    assert total == n


def decision_boundary_stack(rs, n, H, W):
    """n frames around one base image and two models, on both sides of every decision of the chained K2 scan: pixel values
    at 0 / 255 with sigma6 from 0 to 255 (r + s and r - s saturate), isolated supra-threshold pixels of excess 1..6 and
    small clusters whose masses cross the bound only together, the same at the image edges and corners, large excursions
    in every third frame.  Model 0 has sigma 0, model 1 sigma6 = 0 .. 252 and 255."""
    base = rs.randint(0, 256, (H, W)).astype(np.int64)
    base[:, : W // 8] = 0            # c, r at the low rail
    base[:, W // 8: W // 4] = 255    # ... and at the high rail
    frames = np.repeat(base[None], n, 0)
    for f in range(n):
        k = rs.randint(100, 500)
        ys, xs = rs.randint(0, H, k), rs.randint(0, W, k)
        frames[f, ys, xs] += rs.choice([-1, 1], k) * rs.randint(1, 7, k)
        for _ in range(20):  # tight clusters whose masses cross the bound only together
            y, x = rs.randint(0, H - 1), rs.randint(0, W - 2)
            frames[f, y, x] += rs.randint(1, 4)
            frames[f, y + rs.randint(0, 2), x + rs.randint(0, 3)] += rs.randint(1, 4)
        for (y, x) in [(0, 0), (0, 1), (1, 0), (H - 1, W - 1), (H - 2, W - 1), (H - 1, W - 2), (0, W - 1), (H - 1, 0)]:
            frames[f, y, x] += rs.randint(-6, 7)
        if f % 3 == 2:  # large excursions: |c - r| up to 255
            ys, xs = rs.randint(0, H, 60), rs.randint(0, W, 60)
            frames[f, ys, xs] = rs.choice([0, 255], 60)
    frames = np.clip(frames, 0, 255).astype(np.uint8)
    sigma = np.zeros((2, H, W), np.uint8)
    sigma[1] = rs.choice([0, 0, 1, 1, 2, 7, 20, 42, 43, 255], (H, W))  # sigma6 = 0 .. 252, 255 (saturated)
    return frames, sigma


def k3_models(rs, H, W):
    """Two models: mu away from the rails (so that + 50 never clips), sigma in {0, 1, 2}."""
    mu = rs.randint(60, 180, (2, H, W)).astype(np.uint8)
    sg = rs.randint(0, 3, (2, H, W)).astype(np.uint8)
    return mu, sg


def k3_scan_frames(rs, mu, sg, models, ndw, chunk_rows=16):
    """One frame per entry of `models` for the K3 zero scan: mu[model] plus noise inside +-6 sigma (the scan proves such
    rows zero), and on top of it
      frame 0: a blob of + 50, radius about H / 4, centred on a lane boundary (x = k * 4 * ndw);
      frames 1, 2: 9-px vertical stripes of + 30 every 40 px (dozens of suspect groups per row: the LDS lists overflow
      at a small budget);
      frame 3: exactly mu;
      every frame but 3: isolated pixels of + 7 .. + 40 -- the four corners, both sides of every lane boundary in rows 0
      and H - 1, both sides of every chunk edge -- dealt out over the frames in turn, and eight pixels exactly 4 or 5
      above mu + 6 sigma (the box sum at which O turns from 0 to 1)."""
    _, H, W = mu.shape
    n = len(models)
    fr = np.empty((n, H, W), np.int64)
    for k, m in enumerate(models):
        s6 = 6 * sg[m].astype(np.int64)
        fr[k] = mu[m].astype(np.int64) + np.floor(rs.uniform(-1, 1, (H, W)) * (s6 + 0.999)).astype(np.int64).clip(-s6, s6)
    lane_px = 4 * ndw
    lanes = W // lane_px
    yy, xx = np.ogrid[:H, :W]
    r = max(H // 4, 1)
    bx = max(lanes // 2, 1) * lane_px if lanes > 1 else W // 2
    fr[0][(yy - H // 2) ** 2 + (xx - bx) ** 2 <= r * r] += 50
    for k in (1, 2):
        if k < n:
            for x in range(7 + 13 * k, W - 9, 40):
                fr[k, :, x:x + 9] += 30
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    for b in range(lane_px, W, lane_px):
        for y in {0, H - 1}:
            spots += [(y, b - 1), (y, b)]
    for e in range(chunk_rows, H, chunk_rows):
        for x in rs.randint(0, W, 6):
            spots += [(e - 1, int(x)), (e, int(x))]
    targets = [k for k in range(n) if k != 3] or [0]
    for i, (y, x) in enumerate(spots):
        fr[targets[i % len(targets)], y, x] += rs.randint(7, 41)
    # the scan's own decision: a lone pixel 4 above mu + 6 sigma gives O = 0 around it ((4 + 4) / 9), one 5 above gives 1
    for k in targets:
        m = models[k]
        for i in range(8):
            y, x = rs.randint(0, H), rs.randint(0, W)
            fr[k, y, x] = int(mu[m, y, x]) + 6 * int(sg[m, y, x]) + 4 + i % 2
    if n > 3:
        fr[3] = mu[models[3]]
    return np.clip(fr, 0, 255).astype(np.uint8)


def quiet_stack(rs, n, H, W, dense=(), band=None, amp=2, blob_from=None):
    """n frames around one base image with noise of +-amp (quiet under sigma = 1), a few dozen excursions of + 5 .. + 12
    per frame, frames `dense` that differ everywhere by + 30, optionally a dense band (frame, y0, y1) and a blob that grows
    from frame blob_from on."""
    base = rs.randint(40, 180, (H, W)).astype(np.int64)
    fr = base[None] + rs.randint(-amp, amp + 1, (n, H, W))
    yy, xx = np.ogrid[:H, :W]
    for f in range(n):
        k = rs.randint(10, 60)
        fr[f, rs.randint(0, H, k), rs.randint(0, W, k)] += rs.randint(5, 13, k)
        if blob_from is not None and f >= blob_from:
            rad = 2 + (f - blob_from) * max(H // 4, 2) // max(n - blob_from, 1)
            fr[f][(yy - H // 2) ** 2 + (xx - W // 3) ** 2 <= rad * rad] += 40
    for f in dense:
        fr[f] += 30
    if band is not None:
        f, y0, y1 = band
        fr[f, y0:y1, ::2] += 25
    return np.clip(fr, 0, 255).astype(np.uint8)
