#!/usr/bin/env python3
"""Writes tests/golden/bellows40l19.npz (the full-size 40l-19 cam1 / cam3 bellows masks, the cam1 fiducial mask and the
two bellows templates, lossless) from a copy of the reference's cam_masks/40l-19 directory, and
tests/golden/bellows40l19_expected.json: what the CPU oracle finds in every stack of the scenes of bellows40l19_scene.py
(the oracle's full-size matchTemplate takes minutes, so it runs once, here).  Build machine only:
    python tests/golden/make_bellows40l19.py <cam_masks/40l-19 directory>"""
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import bellows40l19_scene as sc  # noqa: E402
from oracle import pyoracle as orc  # noqa: E402


def grey(path):
    return np.array(Image.open(path).convert("L"))


def main(src):
    np.savez_compressed(os.path.join(HERE, "bellows40l19.npz"),
                        cam0_bellows_mask=grey(os.path.join(src, "cam1_bellows_mask.bmp")),
                        cam0_mask=grey(os.path.join(src, "cam1_mask.bmp")),
                        cam1_bellows_mask=grey(os.path.join(src, "cam3_bellows_mask.bmp")),
                        cam0_template=grey(os.path.join(src, "cam1_bellows_template.png")),
                        cam1_template=grey(os.path.join(src, "cam3_bellows_template.png")))
    fx = sc.fixture()
    orc.build()
    out = {"W": sc.W, "H": sc.H, "F": sc.F, "C": sc.C, "kinds": sc.KINDS, "stacks": []}
    for cam in range(sc.C):
        mu, sg = orc.welford(sc.training(fx, cam))
        for e in range(len(sc.KINDS)):
            fr = sc.stack(fx, e, cam)
            a = orc.Analyzer(fr, mu, sg, 2 * sc.NTRAIN, fid_mask=fx["cam0_mask"] if cam == 0 else None,
                             bel_mask=fx["cam%d_bellows_mask" % cam], bel_template=fx["cam%d_template" % cam])
            staged, state, bubbles = a.any_cam_analysis()
            a.close()
            row = {"event": e, "cam": cam, "kind": sc.KINDS[e], "staged": staged, "state": state,
                   "bubbles": [[[d[k] for k in "xywh"] for d in b["desc"]] for b in bubbles]}
            print(json.dumps(row), flush=True)
            out["stacks"].append(row)
    with open(os.path.join(HERE, "bellows40l19_expected.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
