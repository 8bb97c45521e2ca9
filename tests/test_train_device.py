"""Device training (abub::TrainOnDevice, Run.train_on_gpu): every camera of a run trained in one pass -- training frames
decoded by abub_png_decode_dev into one slab, the entropy veto of every (camera, event) pair from one abub_pair_hist_dev
launch, one abub_train_dev per camera -- must give byte for byte what the host Trainer (Run.train) gives: mu, sigma,
TrainingSetSize and status, on clean runs and on every irregular case the host path has a rule for."""
import os
import shutil
import zipfile

import numpy as np
import pytest
from PIL import Image

from autobub3hs_amd import host, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def write_run(root, W=320, H=128, nev=5, ncams=2, F=4, ext="png", seed=0, edit=None):
    """A run on disk: events 0..nev-1, frames cam<c>_image<30+k>.<ext> under <event>/Images; `edit(e, c, k, img, path)`
    may change a frame (return the image to save, or None to skip the file) -- it is called before the file is written."""
    rd = os.path.join(root, "20200925_%d" % seed)
    for e in range(nev):
        for c in range(ncams):
            spec = synth.random_spec(W, H, 41, 500 + 10 * seed + e, c, p_none=0.2, margin=20)
            st = synth.render_event(W, H, spec, 500 + 10 * seed + e, c)[:F]
            d = os.path.join(rd, str(e), "Images")
            os.makedirs(d, exist_ok=True)
            for k in range(F):
                path = os.path.join(d, f"cam{c}_image{30 + k}.{ext}")
                img = st[k] if edit is None else edit(e, c, k, st[k], path)
                if img is not None:
                    Image.fromarray(img).save(path)
    return rd


def zip_run(rd, compress):
    path = rd + ".zip"
    root = os.path.dirname(rd)
    with zipfile.ZipFile(path, "w", compression=compress) as z:
        for dp, dn, fn in os.walk(rd):
            rel = os.path.relpath(dp, root)
            z.writestr(rel + "/", b"")
            for f in sorted(fn):
                z.write(os.path.join(dp, f), os.path.join(rel, f))
    return path


def moving_object(img):
    out = img.copy()
    out[20:60, 40:120] = 255  # between frames 0 and 1: the pair's entropy is far above the veto threshold
    return out


def compare(kind, src, ncams, shape, image_format="cam%d_image%u.png", gpu_decoded=None):
    """train_on_gpu against train(cam) for every camera; returns the device results.  gpu_decoded: the number of frames
    the GPU decoder must have decoded (None: not checked)"""
    dev_run = host.Run(kind, src, "Images", image_format)
    got = dev_run.train_on_gpu(ncams, shape=shape)
    assert dev_run.train_path == "device"
    if gpu_decoded is not None:
        assert dev_run.train_stats["frames_gpu_decoded"] == gpu_decoded, dev_run.train_stats
    dev_run.close()
    host_run = host.Run(kind, src, "Images", image_format)
    for c in range(ncams):
        st, tss, mu, sg = host_run.train(c, shape=shape)
        gst, gtss, gmu, gsg = got[c]
        assert (gst, gtss) == (st, tss), (c, (gst, gtss), (st, tss))
        if st == 0:
            assert np.array_equal(gmu, mu) and np.array_equal(gsg, sg), c
    host_run.close()
    return got


def test_clean_run_matches_host_and_oracle(tmp_path, oracle):
    W, H = 320, 128
    rd = write_run(str(tmp_path), W, H)
    got = compare("raw", rd + "/", 2, (H, W), gpu_decoded=20)
    for c in range(2):
        tr = []
        for e in range(5):
            tr += [np.asarray(Image.open(os.path.join(rd, str(e), "Images", f"cam{c}_image{30 + k}.png"))) for k in (0, 1)]
        mu, sg = oracle.welford(np.stack(tr))
        assert got[c][:2] == (0, 10) and np.array_equal(got[c][2], mu) and np.array_equal(got[c][3], sg)


def test_vetoed_events(tmp_path):
    rd = write_run(str(tmp_path), edit=lambda e, c, k, img, p: moving_object(img) if k == 1 and e in (1, 3) else img)
    got = compare("raw", rd + "/", 2, (128, 320))
    assert [g[1] for g in got] == [6, 6]


def test_event_folder_without_frames(tmp_path):
    """event 2's directory is there (the run lists it) but holds no frames; event 3 has no frames of camera 1"""
    rd = write_run(str(tmp_path), edit=lambda e, c, k, img, p: None if (e == 3 and c == 1) else img)
    shutil.rmtree(os.path.join(rd, "2", "Images"))
    got = compare("raw", rd + "/", 2, (128, 320))
    assert [g[1] for g in got] == [8, 6]


def test_corrupt_frame_beside_a_frame_of_another_size(tmp_path):
    """event 1 / camera 0: frame 0 is truncated, frame 1 is of another size -- the host path skips the event as corrupt
    (the size of the other frame never matters) and trains on the rest"""
    def edit(e, c, k, img, path):
        if (e, c) == (1, 0):
            if k == 1:
                return np.ascontiguousarray(img[:64, :160])
            if k == 0:
                Image.fromarray(img).save(path)
                raw = open(path, "rb").read()
                open(path, "wb").write(raw[: len(raw) // 2])
                return None
        return img

    rd = write_run(str(tmp_path), edit=edit)
    got = compare("raw", rd + "/", 2, (128, 320))
    assert [g[:2] for g in got] == [(0, 8), (0, 10)]


def test_truncated_training_frame(tmp_path):
    def edit(e, c, k, img, path):
        if (e, c, k) == (1, 0, 0):
            Image.fromarray(img).save(path)
            raw = open(path, "rb").read()
            open(path, "wb").write(raw[: len(raw) // 2])
            return None
        return img

    rd = write_run(str(tmp_path), edit=edit)
    got = compare("raw", rd + "/", 2, (128, 320))
    assert [g[1] for g in got] == [8, 10]


def test_sixteen_bit_png_frame_takes_the_host_decoder(tmp_path):
    def edit(e, c, k, img, path):
        if (e, c, k) == (2, 0, 1):
            Image.fromarray(img.astype(np.uint16) * 257).save(path)  # 16-bit grey: the GPU walk refuses it
            return None
        return img

    rd = write_run(str(tmp_path), edit=edit)
    compare("raw", rd + "/", 2, (128, 320))


def test_bmp_series(tmp_path):
    rd = write_run(str(tmp_path), ext="bmp")
    got = compare("raw", rd + "/", 2, (128, 320), image_format="cam%d_image%u.bmp")
    assert [g[0] for g in got] == [0, 0]


@pytest.mark.parametrize("compress", [zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED])
def test_zip_archives(tmp_path, compress):
    rd = write_run(str(tmp_path), edit=lambda e, c, k, img, p: moving_object(img) if (e, k) == (4, 1) else img)
    got = compare("zip", zip_run(rd, compress), 2, (128, 320), gpu_decoded=20)
    assert [g[1] for g in got] == [8, 8]


def test_width_not_a_multiple_of_four(tmp_path):
    W, H = 322, 96
    rd = write_run(str(tmp_path), W=W, H=H)
    got = compare("raw", rd + "/", 2, (H, W))
    assert [g[0] for g in got] == [0, 0]


def test_camera_with_every_pair_vetoed_beside_one_that_trains(tmp_path):
    rd = write_run(str(tmp_path), edit=lambda e, c, k, img, p: moving_object(img) if (c, k) == (1, 1) else img)
    got = compare("raw", rd + "/", 2, (128, 320))
    assert (got[0][0], got[0][1]) == (0, 10) and got[1][0] == -7
