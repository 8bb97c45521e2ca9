"""What the two GPU encoders share: the kernel that places the files of a call, at the frame counts where its scan across
files changes rounds and with source and capacity errors among many files; and the redo of a batch whose files outgrow their
first reservation, through abub3hs --repack-gpu and --unpack-gpu against the host routes, file by file."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import enclayout
from autobub3hs_amd import _lib, hip, host
from enclayout import E_CAP, E_SRC, align16, check_layout, expected_layout, scatter, tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
RUN_ID = "20200925_1"
ENCODERS = {"abf": (hip.abf_encode, host.abf_encode, "abub_abf_file_bound"),
            "png": (hip.png_encode, host.png_huff_encode, "abub_png_file_bound")}
W0, H0 = 64, 3


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def many():
    """300 frames of 64 x 3, flat ones and noise in no regular order, with both host encoders' files: made once, never changed"""
    rs = np.random.RandomState(19)
    imgs = [np.full((H0, W0), i % 251, np.uint8) if rs.randint(0, 2) else rs.randint(0, 256, (H0, W0)).astype(np.uint8)
            for i in range(300)]
    want = {k: [enc(im) for im in imgs] for k, (_, enc, _) in ENCODERS.items()}
    for files in want.values():
        assert len({len(f) for f in files}) >= 2  # (file lengths differ)
    return imgs, want


@pytest.mark.parametrize("n", [255, 256, 257])
@pytest.mark.parametrize("which", sorted(ENCODERS))
def test_placing_across_scan_rounds(many, which, n):
    fn, _, bound = ENCODERS[which]
    imgs, want = many[0][:n], many[1][which][:n]
    buf, offs = scatter(imgs, np.random.RandomState(n))
    room = n * align16(getattr(_lib.lib(), bound)(W0, H0)) + 64
    files, total, out = enclayout.encode(fn, buf, offs, W0, H0, room)
    assert (files[:, 2] == 0).all(), files
    check_layout(files, total, out, want, [True] * n)


@pytest.mark.parametrize("which", sorted(ENCODERS))
def test_source_and_capacity_errors_among_300_files(many, which):
    fn, _, bound = ENCODERS[which]
    imgs, n = many[0], 300
    buf, offs = scatter(imgs, np.random.RandomState(300))
    offs[[7, 290]] = len(buf) - W0 * H0 + 1  # one byte too late to fit
    want = [b"" if f in (7, 290) else w for f, w in enumerate(many[1][which])]
    at, end = expected_layout([len(w) for w in want])
    cap = at[280] + len(want[280]) - 1
    status = [E_SRC if f in (7, 290) else E_CAP if f >= 280 else 0 for f in range(n)]
    room = n * align16(getattr(_lib.lib(), bound)(W0, H0))
    assert end <= room
    files, total, out = enclayout.encode(fn, buf, offs, W0, H0, room, out_cap=cap)
    assert list(files[:, 2]) == status
    assert total == end
    check_layout(files, total, out, want, [s == 0 for s in status])


def write_run(root, frames, save):
    """events x cameras x frames as a run directory; frames[e][c][k] is an image, save(path, image) writes its file"""
    rd = os.path.join(root, RUN_ID)
    for e, cams in enumerate(frames):
        d = os.path.join(rd, str(e), "Images")
        os.makedirs(d)
        for c, stack in enumerate(cams):
            for k, img in enumerate(stack):
                save(os.path.join(d, f"cam{c}_image{30 + k}.png"), img)
    with open(os.path.join(rd, RUN_ID + ".txt"), "w") as f:
        for e in range(len(frames)):
            f.write(f"{RUN_ID} {e} a b c d e f g h i\n")
    return rd


def cli(env, *args):
    r = subprocess.run([EXE] + list(args), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def run_env(batch):
    env = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="4", ABUB_REPACK_BATCH=str(batch))
    env.pop("ABUB_GPU_DECODE", None)
    return env


def same_trees(a, b, nfiles):
    ta, tb = tree(a), tree(b)
    assert sorted(ta) == sorted(tb) and len(ta) == nfiles + 1
    for name in ta:
        assert ta[name] == tb[name], name


def test_repack_gpu_regrows_a_batch_whose_files_outgrow_their_pngs(tmp_path):
    """frames of one noise row repeated: a PNG of 224 bytes, a packed file of 6,816"""
    W, H, F = 96, 64, 6
    rs = np.random.RandomState(2)
    frames = [[[np.ascontiguousarray(np.broadcast_to(rs.randint(0, 256, W).astype(np.uint8), (H, W))) for _ in range(F)]
               for _ in range(2)] for _ in range(2)]
    rd = write_run(str(tmp_path / "data"), frames, lambda path, img: Image.fromarray(img).save(path))
    first8 = frames[0][0] + frames[0][1][:2]  # the first batch, in event, camera and frame order
    pngs = sum(os.path.getsize(os.path.join(rd, "0", "Images", f"cam{c}_image{30 + k}.png")) for c, k in
               [(0, k) for k in range(F)] + [(1, 0), (1, 1)])
    packed = sum(len(host.abf_encode(im)) for im in first8)
    assert packed > 2 * pngs + 8192, (packed, pngs)
    env, data = run_env(8), os.path.dirname(rd)
    a, b = str(tmp_path / "A"), str(tmp_path / "B")
    cli(env, "-d", data, "-r", RUN_ID, "--repack", a)
    lines = cli(env, "-d", data, "-r", RUN_ID, "--repack", b, "--repack-gpu")
    same_trees(a, b, 2 * 2 * F)
    gpu = [l for l in lines if l.startswith("repack-gpu: ")]
    assert len(gpu) == 1 and "3 batches" in gpu[0], lines
    assert any(l.startswith("repack: ") and "0 not written" in l for l in lines), lines


def test_unpack_gpu_regrows_a_batch_whose_files_outgrow_their_packed_frames(tmp_path):
    """flat frames of 1280 x 16: a packed file of 800 bytes, a Huffman-only PNG of 2,674"""
    W, H, F = 1280, 16, 8
    frames = [[[np.full((H, W), 10 + 40 * e + 20 * c + k, np.uint8) for k in range(F)] for c in range(2)] for e in range(2)]
    rd = write_run(str(tmp_path / "data"), frames, lambda path, img: Image.fromarray(img).save(path))
    first16 = frames[0][0] + frames[0][1]
    packed = sum(len(host.abf_encode(im)) for im in first16)
    pngs = sum(len(host.png_huff_encode(im)) for im in first16)
    assert pngs > 2 * packed + 8192, (pngs, packed)
    env = run_env(16)
    p, a, b = str(tmp_path / "P"), str(tmp_path / "A"), str(tmp_path / "B")
    cli(env, "-d", os.path.dirname(rd), "-r", RUN_ID, "--repack", p)
    cli(env, "-d", p, "-r", RUN_ID, "--unpack", a)
    lines = cli(env, "-d", p, "-r", RUN_ID, "--unpack", b, "--unpack-gpu")
    same_trees(a, b, 2 * 2 * F)
    gpu = [l for l in lines if l.startswith("unpack-gpu: ")]
    assert len(gpu) == 1 and "2 batches" in gpu[0], lines
