"""abub3hs --survey --survey-gpu / Run.survey(device=0) against the host route and against the numpy restatement
(tests/surveyref.py), on the damaged run of tests/test_survey_abi.py and a clean copy, from every source form: the same
bytes; with each opt-in decoder knob; in batches of 7; the counters that show that the kernel measured the frames; a width
outside the decoders' gate; the CLI's exit statuses and lines."""
import os
import shutil

import numpy as np
import pytest

import pngadam7 as a7
import pngtypes as pt
from autobub3hs_amd import host
from test_survey_abi import (H, NCAMS, RUN_ID, TOTAL, W, clean, damaged, expected_report, make_survey_run,  # noqa: F401
                             survey_cli)

pytestmark = pytest.mark.gpu

KNOBS = ("ABUB_GPU_BMP", "ABUB_GPU_UNZIP", "ABUB_GPU_PNG_TYPES", "ABUB_GPU_PNG_ADAM7", "ABUB_GPU_DECODE", "ABUB_SURVEY_BATCH")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def survey(src, name, device=None, path=None):
    run = src.open(name)
    try:
        return run.survey(path, nthreads=4, ncams=NCAMS, device=device)
    finally:
        run.close()


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_device_route_writes_the_host_routes_bytes(damaged, clean, tmp_path, monkeypatch):  # noqa: F811
    set_env(monkeypatch, {})
    for (src, frames), rc, not_ok in ((damaged, 1, 4), (clean, 0, 0)):
        want, models = expected_report(src.rd, frames)
        assert all(m is not None for m in models) and " sigma_zero_share -" not in want and " moved_share_median -" not in want
        for name in src.cli:
            cpu, text_cpu = survey(src, name)
            out = str(tmp_path / f"{name}_{rc}.txt")
            gpu, text_gpu = survey(src, name, device=0, path=out)
            assert text_cpu == want and text_gpu == want == open(out).read(), name
            assert cpu["rc"] == gpu["rc"] == rc and gpu["ok"] == TOTAL - not_ok and cpu["device"] == -1
            assert gpu["device"] == 0 and (gpu["W"], gpu["H"]) == (W, H) and gpu["batches"] == 1 and gpu["model_cams"] == NCAMS
            assert gpu["frames_kernel"] == gpu["ok"] and gpu["frames_kernel"] + gpu["frames_host_route"] == gpu["frames"] == TOTAL
            if name in ("dir", "packed") and not not_ok:
                # a condition: the kernel measured every frame, the GPU decoders decoded every one of them
                assert gpu["frames_kernel"] == TOTAL and gpu["frames_host_route"] == 0 and gpu["host_decoded"] == 0
                assert gpu["gpu_png_decoded" if name == "dir" else "gpu_unpacked"] == TOTAL
            if name == "bmp" and not not_ok:
                assert gpu["host_decoded"] == TOTAL and gpu["gpu_bmp_decoded"] == 0  # (BMP files stay with the reading threads)


def test_each_decoder_knob_gives_the_same_bytes(clean, damaged, tmp_path, monkeypatch):  # noqa: F811
    src, frames = clean
    want, _ = expected_report(src.rd, frames)
    set_env(monkeypatch, {"ABUB_GPU_BMP": "1"})
    gpu, text = survey(src, "bmp", device=0)
    assert text == want and gpu["gpu_bmp_decoded"] == TOTAL and gpu["frames_kernel"] == TOTAL
    set_env(monkeypatch, {"ABUB_GPU_UNZIP": "1"})
    gpu, text = survey(src, "deflated", device=0)
    assert text == want and gpu["frames_gpu_unzipped"] > 0 and gpu["frames_kernel"] == TOTAL
    set_env(monkeypatch, {"ABUB_GPU_DECODE": "0"})
    assert survey(src, "dir", device=0)[1] == want
    dsrc, dframes = damaged
    dwant, _ = expected_report(dsrc.rd, dframes)
    for env in ({"ABUB_GPU_BMP": "1"}, {"ABUB_GPU_UNZIP": "1"}):
        set_env(monkeypatch, env)
        for name in ("bmp", "deflated"):
            assert survey(dsrc, name, device=0)[1] == dwant, (env, name)
    # a 16-bit, an RGB and an interlaced frame among the frames: the same pixels, so the same report
    root = str(tmp_path / "typed")
    rd = os.path.join(root, RUN_ID)
    shutil.copytree(src.rd, rd)
    rs = np.random.RandomState(3)
    k16, krgb, ka7 = (0, 0, "cam0_image35.png"), (1, 1, "cam1_image30.png"), (2, 0, "cam0_image39.png")
    grey = lambda k: frames[k].astype(np.uint16)  # noqa: E731
    files = {k16: pt.make_png((grey(k16) << 8)[:, :, None] | rs.randint(0, 256, (H, W, 1)).astype(np.uint16), 0, 16, rs.randint(0, 5, H)),
             krgb: pt.make_png(np.repeat(grey(krgb)[:, :, None], 3, axis=2), 2, 8, rs.randint(0, 5, H)),
             ka7: a7.make_adam7(grey(ka7)[:, :, None], 0, 8, [rs.randint(0, 5, H) for _ in range(7)])}
    for (e, c, name), data in files.items():
        assert np.array_equal(host.imdecode(data), frames[(e, c, name)])
        open(os.path.join(rd, str(e), "Images", name), "wb").write(data)
    run = lambda: host.Run("raw", rd + "/", "Images")  # noqa: E731
    for env, on_host in (({}, 3), ({"ABUB_GPU_PNG_TYPES": "1"}, 1), ({"ABUB_GPU_PNG_ADAM7": "1"}, 2),
                         ({"ABUB_GPU_PNG_TYPES": "1", "ABUB_GPU_PNG_ADAM7": "1"}, 0)):
        set_env(monkeypatch, env)
        r = run()
        try:
            gpu, text = r.survey(nthreads=4, ncams=NCAMS, device=0)
        finally:
            r.close()
        assert text == want, env
        assert gpu["host_decoded"] == on_host and gpu["gpu_png_decoded"] == TOTAL - on_host and gpu["frames_kernel"] == TOTAL, (env, gpu)


def test_batches_of_seven_give_the_same_bytes(damaged, clean, monkeypatch):  # noqa: F811
    """The rule: a batch is seven rows (missing ones counted); the reference frames in front of it are read again into
    slots of their own, so the number of batches is ceil(rows / 7) exactly"""
    for src, frames in (damaged, clean):
        want, _ = expected_report(src.rd, frames)
        for name in ("dir", "deflated", "packed"):
            set_env(monkeypatch, {"ABUB_SURVEY_BATCH": "7"})
            gpu, text = survey(src, name, device=0)
            assert text == want, name
            assert gpu["batches"] == (TOTAL + 6) // 7 and 0 < gpu["reread"] <= 2 * gpu["batches"]
            set_env(monkeypatch, {"ABUB_SURVEY_BATCH": "1"})
            gpu, text = survey(src, name, device=0)
            assert text == want and gpu["batches"] == TOTAL, name


def test_a_width_outside_the_gate_takes_the_host_route_whole(tmp_path, monkeypatch):
    set_env(monkeypatch, {})
    rd, frames = make_survey_run(str(tmp_path / "data"), damaged=False, w=42)
    want, _ = expected_report(rd, frames, w=42)
    run = host.Run("raw", rd + "/", "Images")
    try:
        gpu, text = run.survey(nthreads=4, ncams=NCAMS, device=0)
    finally:
        run.close()
    assert text == want and gpu["rc"] == 0
    assert gpu["device"] == -1 and gpu["frames_kernel"] == 0 and gpu["frames_host_route"] == TOTAL and gpu["batches"] == 0 and gpu["W"] == 42


def test_cli_on_the_device_route(damaged, clean, tmp_path):  # noqa: F811
    for (src, frames), rc in ((damaged, 1), (clean, 0)):
        want, _ = expected_report(src.rd, frames)
        for name in ("dir", "stored", "packed"):
            a, text_a = survey_cli(src.cli[name], str(tmp_path / f"a_{name}_{rc}.txt"))
            b, text_b = survey_cli(src.cli[name], str(tmp_path / f"b_{name}_{rc}.txt"), "--survey-gpu")
            assert a.returncode == b.returncode == rc, a.stderr + b.stderr
            assert text_a == text_b == want, name
            la, lb = [l for l in a.stdout.splitlines() if l.startswith("survey")], [l for l in b.stdout.splitlines() if l.startswith("survey")]
            assert len(la) == 1 and len(lb) == 2 and la[0].rsplit("; ", 1)[0] == lb[0].rsplit("; ", 1)[0]
            assert lb[1].startswith(f"survey-gpu: {TOTAL - 4 * rc} frames measured on GPU 0 "), lb[1]
            # Run.survey agrees with the CLI
            assert survey(src, name, device=0)[1] == text_b
