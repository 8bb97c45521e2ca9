"""The GPU PNG decoder (abub_png_decode_dev) on the hand-written streams of test_png_crafted_streams: what RFC 1951 allows and
no compressor emits.  One batch per geometry holds every case between two copies of a good zlib-made frame; all inflates run
before any unfilter, so a refused stream that wrote past its own raw buffer shows as wrong pixels in a neighbour.  Accepted
cases: status 0 and Pillow's pixels of the same file.  Refused cases: the documented status of include/abub_hip.h.  The same
batches once more through the one-wave route (ABUB_PNG_WAVES=1) in a fresh process.  Every comparison is exact."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_png_crafted_streams import SMALL, WIDE, crafted_cases, pillow_pixels  # noqa: E402

pytestmark = pytest.mark.gpu


def status_codes():
    text = open(os.path.join(ROOT, "include", "abub_hip.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define ABUB_PNG_E_(\w+) (\d+)", text)}


def good_frame(W, H):
    from test_gpu_png import images, make_png
    rs = np.random.RandomState(W + H)
    img = images(rs, W, H)["smooth+noise"]
    return make_png(img, rs.randint(0, 5, H), 6)[0], img


def decode_batches():
    """-> {geometry: (cases, good image, pixels [2n + 1, H, W], status [2n + 1])}: good, case 0, good, case 1, ..., good"""
    import torch
    from autobub3hs_amd import hip
    res = {}
    for W, H in (SMALL, WIDE):
        cases = [c for c in crafted_cases() if (c.W, c.H) == (W, H)]
        good, img = good_frame(W, H)
        files = [good]
        for c in cases:
            files += [c.png, good]
        out, st = hip.png_decode(files, W, H)
        torch.cuda.synchronize()
        res[(W, H)] = (cases, img, out.cpu().numpy(), st)
    return res


def summary(res):
    """what the two routes must agree on: every status and a digest of every pixel of each batch"""
    return {f"{W}x{H}": {"status": [int(v) for v in st], "pixels": hashlib.sha256(px.tobytes()).hexdigest()}
            for (W, H), (_, _, px, st) in res.items()}


@pytest.fixture(scope="module")
def decoded():
    return decode_batches()


def test_every_case_is_in_a_batch(decoded):
    assert sum(len(cases) for cases, _, _, _ in decoded.values()) == len(crafted_cases())


def test_neighbours_of_every_case_stay_intact(decoded):
    for cases, img, px, st in decoded.values():
        for k in range(0, 2 * len(cases) + 1, 2):
            assert st[k] == 0 and np.array_equal(px[k], img), (cases[min(k // 2, len(cases) - 1)].name, k, st[k])


def test_accepted_streams_decode_to_pillow_s_pixels(decoded):
    for cases, _, px, st in decoded.values():
        for k, c in enumerate(cases):
            if c.accepts:
                assert st[2 * k + 1] == 0, (c.name, st[2 * k + 1])  # (a refusal would silently cost the GPU route)
                assert np.array_equal(px[2 * k + 1], pillow_pixels(c.png)), c.name


def test_refused_streams_carry_the_documented_status(decoded):
    """D', E', H: an invalid code in the data; I': the distance is noted when the match is placed and reported at the end of
    the stream, in front of the size and checksum checks; J+: the pass that would write byte H*(W+1) + 1; J-: the end of the
    stream; the three headers: before any block is read."""
    codes = status_codes()
    for cases, _, px, st in decoded.values():
        for k, c in enumerate(cases):
            if not c.accepts:
                assert st[2 * k + 1] != 0, c.name
                assert c.code is not None and st[2 * k + 1] == codes[c.code], (c.name, st[2 * k + 1], c.code)
                assert not px[2 * k + 1].any(), c.name  # (a refused frame is left to the host decoder: nothing is written)


def test_one_wave_route_gives_the_same_statuses_and_pixels(decoded):
    """ABUB_PNG_WAVES=1 (k_png_inflate<false>: one wave parses and writes) is read once per process: one fresh child decodes
    the same batches and reports statuses and a digest of the pixels."""
    env = dict(os.environ, ABUB_PNG_WAVES="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == summary(decoded)


if __name__ == "__main__":
    print(json.dumps(summary(decode_batches())))
