"""Hand-built stacks at the edges where a batched restatement of the trigger search and the localiser goes wrong: bubbles on
the borders and corners, components larger than a frame or than K4b's LDS path, whole-frame steps, saturated and dead
pixels, degenerate models, and stack lengths around the pipeline's lazy frame blocks.  Shared by the CPU pins
(test_oracle_edges.py) and the GPU parity tests (test_gpu_edges.py); integer-only, built on autobub3hs_amd.synth."""
import numpy as np

from autobub3hs_amd import synth

# stack lengths around every F-dependent branch of host/pipeline.cpp: F < 5 (too short), F == 5 (localiser refuses),
# F <= 8 (one frame block), 9 / 10 (lazy, but the first block reaches the end), more blocks from 13 on
STACK_LENGTHS = [1, 2, 3, 5, 6, 8, 9, 10, 13, 17, 41, 64]


def lazy_blocks(F, block0=None, step=None):
    """First frames of the trigger search's frame blocks as host/pipeline.cpp plans them (ABUB_PIPE_LAZY=1), with the
    end of the stack as the last entry: block k covers frames [b[k], b[k + 1])."""
    first = block0 if block0 else F // 2 + 4
    step = step if step else max(4, F // 5)
    b = [1]
    if F > 8:
        x = min(first + 1, F)
        while x < F and len(b) < 32:
            b.append(x)
            x += step
    b.append(max(F, 1))
    return b


def trigger_positions(F):
    """Frames a bubble appears at: the first frame the search may accept (2), the frames around every block boundary (the
    first boundary from two frames before it, so that the look-ahead crosses it), the middle frame F/2 + 4, the last
    frame the look-ahead can confirm (F - 3) and the two whose look-ahead runs past the end (F - 2, F - 1)."""
    inner = lazy_blocks(F)[1:-1]
    cand = {2, F // 2 + 4, F - 3, F - 2, F - 1}
    for k, b in enumerate(inner):
        cand |= {b - 2, b - 1, b} if k == 0 else {b - 1, b}
    return sorted(t for t in cand if 2 <= t < F)


def trigger_stacks(W, H, F, seed=0):
    """-> (frames u8 [E, F, H, W], onsets): one stack per trigger_positions(F) with a bubble growing from that frame on,
    then one quiet stack (onset None)."""
    onsets = trigger_positions(F) + [None]
    out = np.zeros((len(onsets), F, H, W), np.uint8)
    for e, t in enumerate(onsets):
        bub = [] if t is None else [(W // 4 + (17 * e) % (W // 2), H // 2, 40 if e % 2 == 0 else -40)]
        out[e] = synth.render_event(W, H, synth.EventSpec(F, t0=t, bubbles=bub), seed + e, 0)
    return out, onsets


def _render(W, H, F, t0, bubbles, seed, flicker=None):
    return synth.render_event(W, H, synth.EventSpec(F, t0=t0, bubbles=bubbles, flicker=flicker), seed, 0).astype(np.int64)


def _grow_from(fr, t0, mask_of_k, add):
    """fr[t0 + k] += add where mask_of_k(k) (int64 stack, in place)."""
    for f in range(t0, fr.shape[0]):
        fr[f] = np.where(mask_of_k(f - t0), fr[f] + add, fr[f])


def edge_scenes(W, H, F=30, t0=12, welford=None):
    """The table of part 1: name -> (frames u8 [F, H, W], mu u8 [H, W], sigma u8 [H, W], tss).  `welford` is the oracle's
    Welford (the model of the quiet training frames, what Trainer computes)."""
    tr = synth.training_pairs(W, H, 8, 0, F)
    mu, sg = welford(tr)
    tss = len(tr)
    yy, xx = np.mgrid[:H, :W]
    out = {}

    def add(name, fr, m=mu, s=sg, t=tss):
        out[name] = (np.clip(fr, 0, 255).astype(np.uint8), np.ascontiguousarray(m, np.uint8),
                     np.ascontiguousarray(s, np.uint8), t)

    # discs centred on each border and each corner (half or a quarter of the disc inside the frame)
    for nm, (cx, cy) in (("left", (0, H // 2)), ("right", (W - 1, H // 2)), ("top", (W // 3, 0)),
                         ("bottom", (2 * W // 3, H - 1)), ("corner_tl", (0, 0)), ("corner_tr", (W - 1, 0)),
                         ("corner_bl", (0, H - 1)), ("corner_br", (W - 1, H - 1))):
        add("border_" + nm, _render(W, H, F, t0, [(cx, cy, 40 if len(nm) % 2 else -40)], 11 + len(out)))
    # a disc that starts inside and grows across the left edge, next to one that stays inside
    add("crossing", _render(W, H, F, t0, [(7, H // 3, 40), (W // 2, H // 2, -40)], 31))
    # a vertical band over every row (taller than the frame), widening by 2 px per frame
    fr = _render(W, H, F, None, [], 32)
    _grow_from(fr, t0, lambda k: (xx >= W // 4) & (xx < W // 4 + 3 + 2 * k), 45)
    add("taller_than_frame", fr)
    # a disc of radius 27 + 1.5 k: more than 2048 foreground pixels in the genesis and every tracking image (K4b's
    # dense-plane path)
    fr = _render(W, H, F, None, [], 33)
    _grow_from(fr, t0, lambda k: (2 * (xx - W // 2)) ** 2 + (2 * (yy - H // 2)) ** 2 <= (54 + 3 * k) ** 2, 40)
    add("large_component", fr)
    # whole-frame steps of +60 / -60 ADU from the trigger on, with a bubble on top: nearly every pixel is foreground in
    # every tracking image
    for nm, d in (("step_up", 60), ("step_down", -60)):
        fr = _render(W, H, F, t0, [(W // 3, H // 2, -d)], 34 + d)
        fr[t0:] += d
        add(nm, fr)
    # saturated and dead pixels: a block at 255 and one at 0 in every frame, a bubble that saturates on a bright plateau
    # (230 + 40), a dead bubble (0) on the background; mu at 255 / 0 over two other blocks
    fr = _render(W, H, F, None, [], 35)
    fr[:, : H // 3, W // 8: W // 8 + 40] = 255
    fr[:, 2 * H // 3:, W // 8 + 60: W // 8 + 100] = 0
    cx1, cx2 = W // 2, 3 * W // 4
    fr[:, :, cx1 - 30: cx1 + 30] = 230
    _grow_from(fr, t0, lambda k: (2 * (xx - cx1)) ** 2 + (2 * (yy - H // 2)) ** 2 <= (4 + 3 * k) ** 2, 40)
    _grow_from(fr, t0, lambda k: (2 * (xx - cx2)) ** 2 + (2 * (yy - H // 2)) ** 2 <= (4 + 3 * k) ** 2, -500)
    m = mu.copy()
    m[H // 2:, W // 3: W // 3 + 30] = 255
    m[: H // 2, W // 3 + 40: W // 3 + 70] = 0
    add("saturated_dead", fr, m)
    # sigma = 0 everywhere (every noise excursion survives the 6 sigma cut)
    add("sigma_zero", _render(W, H, F, t0, [(W // 2, H // 2, 40)], 36), s=np.zeros_like(sg))
    # 6 sigma clipped at 255: sigma 43 / 60 / 255 over the left half (and 42, just below the clip, in a strip), where a
    # 0 -> 255 flash and a bubble must leave nothing; a bubble on the right half is found as usual
    fr = _render(W, H, F, t0, [(W // 5, H // 2, 40), (3 * W // 4, H // 2, -40)], 37)
    fr[:t0, H // 4: 3 * H // 4, W // 10: W // 10 + 24] = 0
    fr[t0:, H // 4: 3 * H // 4, W // 10: W // 10 + 24] = 255
    s = sg.copy()
    s[:, : W // 2] = np.where(xx[:, : W // 2] % 3 == 0, 43, np.where(xx[:, : W // 2] % 3 == 1, 60, 255))
    s[:, W // 2 - 4: W // 2] = 42
    add("sigma_clipped", fr, s=s)
    # a camera whose every frame is the same constant image, with its own (constant, sigma 0) model
    const = np.full((F, H, W), 77, np.int64)
    add("constant_camera", const, m=np.full((H, W), 77, np.uint8), s=np.zeros((H, W), np.uint8))
    return out
