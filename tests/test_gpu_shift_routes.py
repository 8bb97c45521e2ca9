"""abub3hs --survey --survey-gpu --survey-shift / Run.survey(device=0, shift=...) against the host route and against the numpy
restatement (tests/shiftref.py), on the moving run of tests/test_shift_abi.py from every source form: the same shift file,
byte for byte, and the survey's report as it is without the flag; with each opt-in decoder knob; in batches of 7 and of 1;
the counters that show that the kernel searched the frames; a width outside the decoders' gate; with the planes."""
import os

import pytest

import shiftref
from autobub3hs_amd import host
from test_shift_abi import (F, FAR, H, MOVED_STACK, NEV, TOTAL, TRUNCATED, W, expected_shift, half_trained, make_shift_run,  # noqa: F401
                            moving, shift_cli)
from test_survey_abi import NCAMS, RUN_ID, survey_cli

pytestmark = pytest.mark.gpu

KNOBS = ("ABUB_GPU_BMP", "ABUB_GPU_UNZIP", "ABUB_GPU_PNG_TYPES", "ABUB_GPU_PNG_ADAM7", "ABUB_GPU_DECODE", "ABUB_SURVEY_BATCH")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def want(moving):  # noqa: F811
    src, frames = moving
    text, models = expected_shift(src.rd, frames, 4)
    assert all(m is not None for m in models)
    return text


def survey(src, name, tmp_path, device=None, **kw):
    """-> (stats, report, shift file)"""
    out = str(tmp_path / f"{name}_{device}.shift.txt")
    run = src.open(name)
    try:
        res, text = run.survey(nthreads=4, ncams=NCAMS, device=device, shift=out, **kw)
    finally:
        run.close()
    return res, text, open(out).read()


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_the_trained_models_see_the_run_move(want):
    """with the models the Trainer made (the moved stack has no first frame, so it trains on the other two events) the file
    says what happened: camera 0 at rest but for the far frame on the edge, camera 1 moved by (2, -1) from event 2 on"""
    lines = want.splitlines()
    rows = [l.split("\t") for l in lines[3:3 + TOTAL]]
    for r in rows:
        key = (int(r[0]), int(r[1]), r[3])
        if key == TRUNCATED:
            assert r[4:] == ["undecodable"] + ["-"] * 6
        else:
            assert r[4:8] == ["ok"] + (["2", "-1", "0"] if key[:2] == MOVED_STACK else ["4", "0", "1"] if key == FAR else ["0", "0", "0"]), r
    assert lines[3 + TOTAL] == f"shift cam 0 frames {F * NEV} at_zero {F * NEV - 1} shifted 1 at_edge 1 max_abs_dx 4 max_abs_dy 0 first_shifted_event 1"
    assert lines[4 + TOTAL] == (f"shift cam 1 frames {F * NEV - 1} at_zero {F * (NEV - 1)} shifted {F - 1} at_edge 0 max_abs_dx 2 "
                                "max_abs_dy 1 first_shifted_event 2")
    assert lines[5 + TOTAL] == f"run frames {TOTAL - 1} shifted {F} at_edge 1"


def test_device_route_writes_the_host_routes_bytes(moving, want, tmp_path, monkeypatch):  # noqa: F811
    set_env(monkeypatch, {})
    src, frames = moving
    for name in src.cli:
        run = src.open(name)
        try:
            plain = run.survey(nthreads=4, ncams=NCAMS, device=0)[1]
        finally:
            run.close()
        cpu, text_cpu, shift_cpu = survey(src, name, tmp_path)
        gpu, text_gpu, shift_gpu = survey(src, name, tmp_path, device=0)
        assert shift_cpu == want and shift_gpu == want, name
        assert text_cpu == text_gpu == plain, name
        assert cpu["shift_frames_kernel"] == 0 and cpu["shift_frames_host"] == TOTAL - 1 and cpu["shift_launches"] == 0
        assert gpu["shift_frames_kernel"] + gpu["shift_frames_host"] == TOTAL - 1 and gpu["batches"] == 1
        assert gpu["shift_frames_kernel"] == gpu["frames_kernel"] == TOTAL - 1 and gpu["shift_launches"] == 1
    for radius in (1, 8):
        expected = expected_shift(src.rd, frames, radius)[0]
        assert survey(src, "dir", tmp_path, device=0, shift_radius=radius)[2] == expected
        assert survey(src, "packed", tmp_path, shift_radius=radius)[2] == expected


def test_the_kernel_searches_every_frame_with_a_model(half_trained, tmp_path, monkeypatch):  # noqa: F811
    """camera 0 does not train: its rows have no surface on either route, and the kernel's counter is camera 1's ok frames"""
    set_env(monkeypatch, {})
    rd, frames = half_trained
    expected, models = expected_shift(rd, frames, 4)
    assert models[0] is None and models[1] is not None
    for device in (None, 0):
        run = host.Run("raw", rd + "/", "Images")
        try:
            res, _ = run.survey(nthreads=4, ncams=NCAMS, device=device, shift=str(tmp_path / "half.txt"))
        finally:
            run.close()
        assert open(str(tmp_path / "half.txt")).read() == expected
        assert res["shift_frames_kernel" if device == 0 else "shift_frames_host"] == F * NEV - 1
        assert res["shift_frames_host" if device == 0 else "shift_frames_kernel"] == 0


def test_each_decoder_knob_gives_the_same_bytes(moving, want, tmp_path, monkeypatch):  # noqa: F811
    src, _ = moving
    for env, name in (({"ABUB_GPU_BMP": "1"}, "bmp"), ({"ABUB_GPU_UNZIP": "1"}, "deflated"), ({"ABUB_GPU_PNG_TYPES": "1"}, "dir"),
                      ({"ABUB_GPU_PNG_ADAM7": "1"}, "dir"), ({"ABUB_GPU_DECODE": "0"}, "dir"), ({"ABUB_GPU_DECODE": "0"}, "packed")):
        set_env(monkeypatch, env)
        gpu, _, shift = survey(src, name, tmp_path, device=0)
        assert shift == want, (env, name)
        assert gpu["shift_frames_kernel"] + gpu["shift_frames_host"] == TOTAL - 1


def test_small_batches_give_the_same_bytes(moving, want, tmp_path, monkeypatch):  # noqa: F811
    src, _ = moving
    for name in ("dir", "deflated", "packed"):
        set_env(monkeypatch, {"ABUB_SURVEY_BATCH": "7"})
        gpu, _, shift = survey(src, name, tmp_path, device=0)
        assert shift == want and gpu["batches"] == (TOTAL + 6) // 7 and gpu["shift_launches"] == gpu["batches"], name
        set_env(monkeypatch, {"ABUB_SURVEY_BATCH": "1"})
        gpu, _, shift = survey(src, name, tmp_path, device=0)
        assert shift == want and gpu["batches"] == TOTAL and gpu["shift_launches"] == TOTAL - 1, name  # (the truncated file has no job)
        assert gpu["shift_frames_kernel"] == TOTAL - 1


def test_the_kernels_counter_on_clean_runs(tmp_path, monkeypatch):
    """a run without damage, from PNG files and from its packed copy: every frame has a model and is the kernel's"""
    from test_survey_abi import Sources
    set_env(monkeypatch, {})
    root = str(tmp_path / "clean")
    rd, frames = make_shift_run(os.path.join(root, "data"), w=W + 4)  # (another width: no file is truncated)
    src = Sources(root, rd)
    expected, models = expected_shift(rd, frames, 4, w=W + 4)
    assert all(m is not None for m in models)
    for name in ("dir", "packed"):
        gpu, _, shift = survey(src, name, tmp_path, device=0)
        assert shift == expected and gpu["rc"] == 0
        assert gpu["shift_frames_kernel"] == gpu["frames_kernel"] == TOTAL and gpu["shift_frames_host"] == 0 and gpu["host_decoded"] == 0


def test_a_width_outside_the_gate_takes_the_host_route_whole(tmp_path, monkeypatch):
    set_env(monkeypatch, {})
    rd, frames = make_shift_run(str(tmp_path / "data"), w=42)
    expected, models = expected_shift(rd, frames, 4, w=42)
    assert all(m is not None for m in models)
    run = host.Run("raw", rd + "/", "Images")
    try:
        gpu, _ = run.survey(nthreads=4, ncams=NCAMS, device=0, shift=str(tmp_path / "s.txt"))
    finally:
        run.close()
    assert open(str(tmp_path / "s.txt")).read() == expected and gpu["rc"] == 0
    assert gpu["device"] == -1 and gpu["shift_frames_kernel"] == 0 and gpu["shift_launches"] == 0 and gpu["shift_frames_host"] == TOTAL


def test_cli_on_the_device_route_and_with_planes(moving, want, tmp_path):  # noqa: F811
    src, _ = moving
    for name in ("dir", "stored", "packed"):
        plain, report_plain = survey_cli(src.cli[name], str(tmp_path / f"plain_{name}.txt"), "--survey-gpu", "--survey-planes",
                                         str(tmp_path / f"planes_plain_{name}"))
        a, report_a, shift_a = shift_cli(src.cli[name], str(tmp_path / f"a_{name}"))
        b, report_b, shift_b = shift_cli(src.cli[name], str(tmp_path / f"b_{name}"), "--survey-gpu", "--survey-planes",
                                         str(tmp_path / f"planes_{name}"))
        assert a.returncode == b.returncode == plain.returncode == 1, a.stderr + b.stderr
        assert shift_a == shift_b == want and report_a == report_b == report_plain, name
        line = [l for l in b.stdout.splitlines() if l.startswith("survey-shift: ")]
        assert len(line) == 1 and f"radius 4, {TOTAL - 1} frames searched on the GPU in 1 launches, 0 on the host" in line[0], b.stdout
        with_flag, without = os.path.join(str(tmp_path / f"planes_{name}"), RUN_ID), os.path.join(str(tmp_path / f"planes_plain_{name}"), RUN_ID)
        assert sorted(os.listdir(with_flag)) == sorted(os.listdir(without)) and len(os.listdir(without)) == 2 * NCAMS + 1
        for f in os.listdir(without):
            assert open(os.path.join(with_flag, f), "rb").read() == open(os.path.join(without, f), "rb").read(), (name, f)
    r = shift_cli(src.cli["dir"], str(tmp_path / "small"), "--survey-gpu", "--survey-shift-radius", "8")[0]
    assert r.returncode == 1
    rd, _ = make_shift_run(str(tmp_path / "tiny"), w=8, h=8)
    r, report, shift = shift_cli(["-d", os.path.dirname(rd), "-r", RUN_ID], str(tmp_path / "tiny_out"), "--survey-gpu")
    assert r.returncode != 0 and "needs frames of at least 9x9, the run's are 8x8" in r.stderr and report is None and shift is None
