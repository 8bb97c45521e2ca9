"""Deterministic full-size 40l-19 bellows scenes (1680 x 1050, C = 2, 41-frame stacks) built from the committed
fixture tests/golden/bellows40l19.npz, autobub3hs_amd.synth and the committed camera sample: camera 0 has the geometry
of the real cam1 (its bellows mask, fiducial mask and 178 x 557 bellows template), camera 1 that of cam3 (bellows mask,
152 x 509 template, no fiducial mask).  Shared by tests/golden/make_bellows40l19.py and tests/test_bellows_batched.py."""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, F, C, NTRAIN = 1680, 1050, 41, 2, 6
T0 = 20           # the bellows template starts to creep at this frame ...
CREEP = 2         # ... one pixel per frame for this many frames
PLACE = [(1486, 158), (1482, 222)]  # rest position (x, y) of the template, inside the bellows mask, per camera
# stacks: (i) creep only, (ii) creep + a bubble in the fiducial region outside the bellows mask, (iii) creep + a bubble
# inside the bellows mask (away from the template), (iv) quiet
KINDS = ["creep", "creep+bubble", "creep+bubble_in_bellows", "quiet"]
BUBBLE = {"creep+bubble": (600, 500), "creep+bubble_in_bellows": (1640, 860)}


def fixture():
    z = np.load(os.path.join(HERE, "bellows40l19.npz"))
    return {k: z[k] for k in z.files}


def texture(cam):
    """the camera sample tiled over the frame: bellows-like structure around the template"""
    img = np.array(Image.open(os.path.join(HERE, "sample_40l19_cam1_image30.png")).convert("L")).astype(np.int32)
    t = np.tile(img, (H // img.shape[0] + 1, W // img.shape[1] + 1))[:H, :W]
    return np.roll(t, 17 * cam, axis=1)


def stack(fx, e, cam):
    """frames [F, H, W] u8 of event e (one of KINDS) on camera cam"""
    from autobub3hs_amd import synth

    kind = KINDS[e]
    spec = synth.EventSpec(F, t0=T0 if kind in BUBBLE else None,
                           bubbles=[(BUBBLE[kind][0], BUBBLE[kind][1], 40)] if kind in BUBBLE else [])
    fr = synth.render_event(W, H, spec, 500 + e, cam).astype(np.int32)
    fr = (fr + texture(cam)) // 2
    tpl = fx["cam%d_template" % cam].astype(np.int32)
    th, tw = tpl.shape
    x0, y0 = PLACE[cam]
    for f in range(F):
        dx = 0 if kind == "quiet" or f < T0 else min(f - T0 + 1, CREEP)
        fr[f, y0:y0 + th, x0 + dx:x0 + dx + tw] = tpl
    return np.clip(fr, 0, 255).astype(np.uint8)


def training(fx, cam):
    from autobub3hs_amd import synth

    tr = synth.training_pairs(W, H, NTRAIN, cam, F).astype(np.int32)
    tr = (tr + texture(cam)[None]) // 2
    tpl = fx["cam%d_template" % cam]
    th, tw = tpl.shape
    x0, y0 = PLACE[cam]
    tr[:, y0:y0 + th, x0:x0 + tw] = tpl
    return np.clip(tr, 0, 255).astype(np.uint8)


def write_masks(fx, d):
    """the masks and templates as the product reads them from a mask directory"""
    Image.fromarray(fx["cam0_bellows_mask"]).save(os.path.join(d, "cam0_bellows_mask.bmp"))
    Image.fromarray(fx["cam0_mask"]).save(os.path.join(d, "cam0_mask.bmp"))
    Image.fromarray(fx["cam1_bellows_mask"]).save(os.path.join(d, "cam1_bellows_mask.bmp"))
    Image.fromarray(fx["cam0_template"]).save(os.path.join(d, "cam0_bellows_template.png"))
    Image.fromarray(fx["cam1_template"]).save(os.path.join(d, "cam1_bellows_template.png"))
