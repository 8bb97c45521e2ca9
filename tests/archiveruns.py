"""What the tests of abub3hs --archive share (test_zip_archive.py on the CPU, test_gpu_archive_routes.py on the GPU): tiny
runs on disk, the command line, and the checks of an archive against the tree the directory route writes."""
import os
import subprocess
import zipfile

import numpy as np
from PIL import Image

import zipref
from autobub3hs_amd import host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
RUN_ID = "20200925_1"


def env(**more):
    e = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="4")
    for k in ("ABUB_GPU_DECODE", "ABUB_ZIP64_FORCE", "ABUB_REPACK_BATCH"):
        e.pop(k, None)
    e.update(more)
    return e


def cli(*args, ok=True, **more):
    r = subprocess.run([EXE] + [str(a) for a in args], env=env(**more), capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, r.stdout + r.stderr
    return r


def make_run(root, W=64, H=48, F=4, nev=3, ncams=2, mixed=True):
    """PNG frames of W x H, a run file, an event directory without frames (9).  mixed: event 1 also has a frame of another
    size, a 16-bit PNG, a frame that is packed already and a truncated file that does not decode, event 2 an empty file.
    -> (run directory, {(event, cam, name): pixels or None for the file that does not decode})"""
    rd = os.path.join(root, RUN_ID)
    frames = {}
    for e in range(nev):
        d = os.path.join(rd, str(e), "Images")
        os.makedirs(d, exist_ok=True)
        for c in range(ncams):
            spec = synth.random_spec(W, H, F, 300 + e, c, margin=10)
            st = synth.render_event(W, H, spec, 300 + e, c)
            for k in range(F):
                name = f"cam{c}_image{30 + k}.png"
                Image.fromarray(st[k]).save(os.path.join(d, name))
                frames[(e, c, name)] = st[k]
    if mixed:
        d = os.path.join(rd, "1", "Images")
        other = np.full((H + 2, W + 4), 9, np.uint8)
        Image.fromarray(other).save(os.path.join(d, "cam0_image31.png"))
        frames[(1, 0, "cam0_image31.png")] = other
        Image.fromarray(frames[(1, 0, "cam0_image32.png")].astype(np.uint16) << 8).save(os.path.join(d, "cam0_image32.png"))
        open(os.path.join(d, "cam1_image30.png"), "wb").write(host.abf_encode(frames[(1, 1, "cam1_image30.png")]))
        victim = os.path.join(d, "cam1_image32.png")
        cut = open(victim, "rb").read()[:120]
        open(victim, "wb").write(cut)
        frames[(1, 1, "cam1_image32.png")] = None
        open(os.path.join(rd, "2", "Images", "cam0_image33.png"), "wb").close()  # an empty file
        frames[(2, 0, "cam0_image33.png")] = None
    with open(os.path.join(rd, RUN_ID + ".txt"), "w") as f:
        for e in range(nev):
            f.write(f"{RUN_ID} {e} a b c d e f g h i\n")
    os.makedirs(os.path.join(rd, "9", "Images"), exist_ok=True)
    return rd, frames


def zip_run(rd, path, compress=zipfile.ZIP_STORED):
    root = os.path.dirname(rd)
    with zipfile.ZipFile(path, "w", compression=compress, allowZip64=True) as z:
        for dp, dn, fn in sorted(os.walk(rd)):
            rel = os.path.relpath(dp, root)
            z.writestr(rel + "/", b"")
            for f in sorted(fn):
                z.write(os.path.join(dp, f), os.path.join(rel, f))


def tree(root):
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(dp, f), root)] = open(os.path.join(dp, f), "rb").read()
    return out


def expected_entries(run_tree, events=("0", "1", "2", "9"), ncams=2):
    """the canonical entries of the archive whose files are `run_tree` (what tree() gives for the directory route's output,
    keys <run>/...): <run>/, the event file, per event its directories and its frames in camera and frame order"""
    text = run_tree.get(f"{RUN_ID}/{RUN_ID}.txt", b"")
    per_event = []
    for ev in events:
        names = sorted(k.split("/")[-1] for k in run_tree if k.startswith(f"{RUN_ID}/{ev}/Images/"))
        ordered = [n for c in range(ncams) for n in names if n.startswith(f"cam{c}")]
        per_event.append((ev, [(n, run_tree[f"{RUN_ID}/{ev}/Images/{n}"]) for n in ordered]))
    return zipref.run_entries(RUN_ID, text, per_event)


def check_archive(path, run_tree, force64=False):
    """`path` is the canonical archive of the files in run_tree: readable by zipfile, the expected names in order, every
    entry's bytes, and byte for byte what tests/zipref.py writes"""
    entries = expected_entries(run_tree)
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
        assert z.namelist() == [n.decode() for n, _ in entries]
        for n, data in entries:
            assert z.read(n.decode()) == data, n
        for info in z.infolist():
            if info.file_size:
                assert (info.header_offset + 30 + len(info.filename) + len(zipref.extra_field(zipref.extra_len(
                    info.header_offset, len(info.filename), info.file_size)))) % 16 == 0, info.filename
    got = open(path, "rb").read()
    assert got == zipref.archive(entries, force64=force64)
    return entries


def check_same_run(zpath, dir_rd):
    """Run(kind="zip") on the archive lists the events and frames and decodes the pixels of the directory copy"""
    a, b = host.Run("zip", zpath, "Images"), host.Run("raw", dir_rd + "/", "Images")
    try:
        assert a.events() == b.events() == ["0", "1", "2", "9"]
        for e in a.events():
            for c in range(2):
                assert a.frames(e, c) == b.frames(e, c)
                for name in b.frames(e, c):
                    ia, ib = a.image(e, name)[1], b.image(e, name)[1]  # (None: the file does not decode)
                    assert (ia is None) == (ib is None), (e, name)
                    assert ia is None or np.array_equal(ia, ib), (e, name)
    finally:
        a.close()
        b.close()
