"""What the tests of the two GPU encoders (hip.abf_encode, hip.png_encode) share: frames scattered over a source buffer, one
call with canaries around `out`, the layout rule of the files (off[0] = 0, off[f + 1] = align16(off[f] + len[f])) and the
check of an output buffer against it; and a directory tree as a dict, for the routes that write files."""
import os

import numpy as np
import torch

CANARY = 0xA5
DEV = "cuda:0"
E_SRC, E_CAP = 1, 2


def align16(v):
    return (v + 15) & ~15


def scatter(imgs, rs):
    """the frames at scattered, unaligned offsets of a random buffer, not in order -> (buffer, offsets)"""
    P = imgs[0].size
    order = rs.permutation(len(imgs))
    offs = np.zeros(len(imgs), np.int64)
    at = 3
    for slot in order:
        at += int(rs.randint(1, 40))
        offs[slot] = at
        at += P
    buf = rs.randint(0, 256, at + 11).astype(np.uint8)
    for o, img in zip(offs, imgs):
        buf[o:o + P] = img.reshape(-1)
    return buf, offs


def encode(fn, buf, offs, W, H, out_bytes, out_cap=None, out=None, scratch=None):
    """one call of fn (hip.abf_encode or hip.png_encode); canaries all over `out` and in front of and behind it ->
    (files, total, out bytes on the host)"""
    pixels = torch.from_numpy(buf).to(DEV)
    whole = torch.full((out_bytes + 512,), CANARY, dtype=torch.uint8, device=DEV) if out is None else out
    files, total, _ = fn(pixels, offs, W, H, out=whole[256:256 + out_bytes], out_cap=out_cap, scratch=scratch)
    torch.cuda.synchronize()
    host_out = whole.cpu().numpy()
    assert (host_out[:256] == CANARY).all() and (host_out[256 + out_bytes:] == CANARY).all(), "written outside out"
    return files, total, host_out[256:256 + out_bytes]


def expected_layout(lens):
    offs, at = [], 0
    for n in lens:
        offs.append(at)
        at = align16(at + n)
    return offs, (offs[-1] + lens[-1] if lens else 0)


def check_layout(files, total, out, want, written):
    """want[f]: the bytes of file f (b"" for a frame that takes no room); written[f]: whether they must be in `out`.  Every
    byte outside the written files is still the canary."""
    offs, end = expected_layout([len(w) for w in want])
    assert list(files[:, 0]) == offs and list(files[:, 1]) == [len(w) for w in want] and total == end
    free = np.ones(len(out), bool)
    for f, (o, w, there) in enumerate(zip(offs, want, written)):
        if there:
            got = out[o:o + len(w)].tobytes()
            if got != w:
                first = next(i for i in range(len(w)) if got[i] != w[i])
                raise AssertionError(f"file {f}: {sum(a != b for a, b in zip(got, w))} of {len(w)} bytes differ, the first at {first}: "
                                     f"{got[first:first + 8].hex()} for {w[first:first + 8].hex()}")
            free[o:o + len(w)] = False
    assert (out[free] == CANARY).all(), "written outside the files"


def tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), "rb").read()
    return out
