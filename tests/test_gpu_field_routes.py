"""abub3hs --survey --survey-gpu --survey-field / Run.survey(device=0, field=...) against the host route and against the numpy
restatement (tests/fieldref.py), on the moving run of tests/test_field_abi.py from every source form: the same field.txt and
.npy files, byte for byte, and the survey's report as it is without the flag; with each opt-in decoder knob; in batches of 7
and of 1; with the surface buffer forced to split; the counters that show that the kernel searched the frames; a width outside
the decoders' gate; together with the planes and the shift file."""
import os

import pytest

from autobub3hs_amd import host
from test_field_abi import (F, NEV, TOTAL, W, check_kinds, expected_field, field_cli, half_trained, make_field_run, moving,  # noqa: F401
                            read_field, same_arrays)
from test_survey_abi import NCAMS, RUN_ID, Sources, survey_cli

pytestmark = pytest.mark.gpu

KNOBS = ("ABUB_GPU_BMP", "ABUB_GPU_UNZIP", "ABUB_GPU_PNG_TYPES", "ABUB_GPU_PNG_ADAM7", "ABUB_GPU_DECODE", "ABUB_SURVEY_BATCH",
         "ABUB_FIELD_CHUNK")


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def want(moving):  # noqa: F811
    src, frames = moving
    text, arrays, models = expected_field(src.rd, frames, 4)
    assert all(m is not None for m in models)
    return text, arrays


def survey(src, name, tmp_path, device=None, **kw):
    """-> (stats, report, field.txt, the arrays, the files' bytes)"""
    out = str(tmp_path / f"{name}_{device}_field")
    run = src.open(name) if isinstance(name, str) else name
    try:
        res, text = run.survey(nthreads=4, ncams=NCAMS, device=device, field=out, **kw)
    finally:
        run.close()
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    return (res, text) + read_field(out) + (files,)


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_the_trained_models_see_the_run_move(want):
    """with the models the Trainer made (the rigid stack has no first frame, so camera 1 trains on the other events) the
    file says what was done to every frame"""
    check_kinds(want[0])


def test_device_route_writes_the_host_routes_bytes(moving, want, tmp_path, monkeypatch):  # noqa: F811
    set_env(monkeypatch, {})
    src, frames = moving
    for name in src.cli:
        run = src.open(name)
        try:
            plain = run.survey(nthreads=4, ncams=NCAMS, device=0)[1]
        finally:
            run.close()
        cpu, text_cpu, field_cpu, arrays_cpu, files_cpu = survey(src, name, tmp_path)
        gpu, text_gpu, field_gpu, arrays_gpu, files_gpu = survey(src, name, tmp_path, device=0)
        assert field_cpu == want[0] and field_gpu == want[0] and same_arrays(arrays_cpu, want[1]) and same_arrays(arrays_gpu, want[1]), name
        assert files_cpu == files_gpu and sorted(files_gpu) == ["cam0_field.npy", "cam1_field.npy", "field.txt"], name
        assert text_cpu == text_gpu == plain, name
        assert cpu["field_frames_kernel"] == 0 and cpu["field_frames_host"] == TOTAL - 1 and cpu["field_launches"] == 0
        assert gpu["field_frames_kernel"] + gpu["field_frames_host"] == TOTAL - 1 and gpu["batches"] == 1
        assert gpu["field_frames_kernel"] == gpu["frames_kernel"] == TOTAL - 1 and gpu["field_launches"] == 1
    for radius in (1, 8):
        text, arrays, _ = expected_field(src.rd, frames, radius)
        got = survey(src, "dir", tmp_path, device=0, field_radius=radius)
        assert got[2] == text and same_arrays(got[3], arrays), radius
        assert survey(src, "packed", tmp_path, field_radius=radius)[4] == got[4], radius


def test_the_kernel_searches_every_frame_with_a_model(half_trained, tmp_path, monkeypatch):  # noqa: F811
    """camera 0 does not train: its rows have no surface on either route, and the kernel's counter is camera 1's ok frames"""
    set_env(monkeypatch, {})
    rd, frames = half_trained
    text, arrays, models = expected_field(rd, frames, 4)
    assert models[0] is None and models[1] is not None
    for device in (None, 0):
        res, _, got, got_arrays, files = survey(None, host.Run("raw", rd + "/", "Images"), tmp_path, device=device)
        assert got == text and same_arrays(got_arrays, arrays) and sorted(files) == ["cam1_field.npy", "field.txt"]
        assert res["field_frames_kernel" if device == 0 else "field_frames_host"] == F * NEV - 1
        assert res["field_frames_host" if device == 0 else "field_frames_kernel"] == 0


def test_each_decoder_knob_gives_the_same_bytes(moving, want, tmp_path, monkeypatch):  # noqa: F811
    src, _ = moving
    for env, name in (({"ABUB_GPU_BMP": "1"}, "bmp"), ({"ABUB_GPU_UNZIP": "1"}, "deflated"), ({"ABUB_GPU_PNG_TYPES": "1"}, "dir"),
                      ({"ABUB_GPU_PNG_ADAM7": "1"}, "dir"), ({"ABUB_GPU_DECODE": "0"}, "dir"), ({"ABUB_GPU_DECODE": "0"}, "packed")):
        set_env(monkeypatch, env)
        gpu, _, text, arrays, _ = survey(src, name, tmp_path, device=0)
        assert text == want[0] and same_arrays(arrays, want[1]), (env, name)
        assert gpu["field_frames_kernel"] + gpu["field_frames_host"] == TOTAL - 1


def test_small_batches_and_a_split_surface_buffer_give_the_same_bytes(moving, want, tmp_path, monkeypatch):  # noqa: F811
    src, _ = moving
    for name in ("dir", "deflated", "packed"):
        set_env(monkeypatch, {"ABUB_SURVEY_BATCH": "7"})
        gpu, _, text, arrays, _ = survey(src, name, tmp_path, device=0)
        assert text == want[0] and same_arrays(arrays, want[1]) and gpu["batches"] == (TOTAL + 6) // 7, name
        assert gpu["field_launches"] == gpu["batches"], name
        set_env(monkeypatch, {"ABUB_SURVEY_BATCH": "1"})
        gpu, _, text, arrays, _ = survey(src, name, tmp_path, device=0)
        assert text == want[0] and same_arrays(arrays, want[1]) and gpu["batches"] == TOTAL, name
        assert gpu["field_launches"] == TOTAL - 1 == gpu["field_frames_kernel"], name  # (the truncated file has no job)
    # one batch whose jobs go to the kernel in calls of 4, 1 and more than there are
    for chunk, launches in (("4", (TOTAL - 1 + 3) // 4), ("1", TOTAL - 1), ("1000", 1)):
        set_env(monkeypatch, {"ABUB_FIELD_CHUNK": chunk})
        gpu, _, text, arrays, _ = survey(src, "dir", tmp_path, device=0)
        assert text == want[0] and same_arrays(arrays, want[1]), chunk
        assert gpu["batches"] == 1 and gpu["field_launches"] == launches and gpu["field_frames_kernel"] == TOTAL - 1, chunk
    set_env(monkeypatch, {"ABUB_FIELD_CHUNK": "3", "ABUB_SURVEY_BATCH": "7"})
    gpu, _, text, arrays, _ = survey(src, "packed", tmp_path, device=0, field_radius=8)
    host_route = survey(src, "packed", tmp_path, field_radius=8)
    assert text == host_route[2] and same_arrays(arrays, host_route[3]) and gpu["field_launches"] > gpu["batches"]


def test_the_kernels_counter_on_clean_runs(tmp_path, monkeypatch):
    """a run without damage, from PNG files and from its packed copy: every frame has a model and is the kernel's"""
    set_env(monkeypatch, {})
    root = str(tmp_path / "clean")
    rd, frames = make_field_run(os.path.join(root, "data"), w=W + 4)  # (another width: plain frames, no file is truncated)
    src = Sources(root, rd)
    text, arrays, models = expected_field(rd, frames, 4, w=W + 4)
    assert all(m is not None for m in models)
    for name in ("dir", "packed"):
        gpu, _, got, got_arrays, _ = survey(src, name, tmp_path, device=0)
        assert got == text and same_arrays(got_arrays, arrays) and gpu["rc"] == 0
        assert gpu["field_frames_kernel"] == gpu["frames_kernel"] == TOTAL and gpu["field_frames_host"] == 0 and gpu["host_decoded"] == 0
        assert f"run frames {TOTAL} blind 0 still {TOTAL} rigid 0 warped 0 local 0\n" in got


def test_a_width_outside_the_gate_takes_the_host_route_whole(tmp_path, monkeypatch):
    """138 columns (as 42, no multiple of 4: no GPU decoder takes the width; 42 itself has no whole cell): the run goes to
    the host whole, and the files are the host route's"""
    set_env(monkeypatch, {})
    rd, frames = make_field_run(str(tmp_path / "data"), w=138, h=140)
    text, arrays, models = expected_field(rd, frames, 4, w=138, h=140)
    assert all(m is not None for m in models)
    gpu, _, got, got_arrays, _ = survey(None, host.Run("raw", rd + "/", "Images"), tmp_path, device=0)
    assert got == text and same_arrays(got_arrays, arrays) and gpu["rc"] == 0
    assert gpu["device"] == -1 and gpu["field_frames_kernel"] == 0 and gpu["field_launches"] == 0 and gpu["field_frames_host"] == TOTAL


def test_a_42_wide_run_is_refused_on_both_routes(tmp_path, monkeypatch):
    """42 columns hold no whole cell: the refusal comes before the route is chosen, the same with and without a device; a
    survey without the field still runs, on the host"""
    set_env(monkeypatch, {})
    rd, frames = make_field_run(str(tmp_path / "data"), w=42, h=140)
    for device in (None, 0):
        run = host.Run("raw", rd + "/", "Images")
        try:
            with pytest.raises(RuntimeError, match="needs frames of at least 136x136, the run's are 42x140"):
                run.survey(nthreads=4, ncams=NCAMS, device=device, field=str(tmp_path / "f"))
            res, _ = run.survey(nthreads=4, ncams=NCAMS, device=device)
        finally:
            run.close()
        assert res["device"] == -1 and not os.path.exists(str(tmp_path / "f"))


def test_cli_on_the_device_route_with_planes_and_shift(moving, want, tmp_path):  # noqa: F811
    src, _ = moving
    for name in ("dir", "stored", "packed"):
        others = lambda tag: ["--survey-gpu", "--survey-planes", str(tmp_path / f"planes_{tag}_{name}"), "--survey-shift",  # noqa: E731
                              str(tmp_path / f"shift_{tag}_{name}.txt")]
        plain, report_plain = survey_cli(src.cli[name], str(tmp_path / f"plain_{name}.txt"), *others("plain"))
        a, report_a, text_a, arrays_a = field_cli(src.cli[name], str(tmp_path / f"a_{name}"))
        b, report_b, text_b, arrays_b = field_cli(src.cli[name], str(tmp_path / f"b_{name}"), *others("with"))
        assert a.returncode == b.returncode == plain.returncode == 1, a.stderr + b.stderr
        assert text_a == text_b == want[0] and same_arrays(arrays_a, want[1]) and same_arrays(arrays_b, want[1]), name
        assert report_a == report_b == report_plain, name
        line = [l for l in b.stdout.splitlines() if l.startswith("survey-field: ")]
        assert len(line) == 1 and f"radius 4, {TOTAL - 1} frames searched on the GPU in 1 launches, 0 on the host" in line[0], b.stdout
        assert open(str(tmp_path / f"shift_with_{name}.txt")).read() == open(str(tmp_path / f"shift_plain_{name}.txt")).read()
        with_flag, without = (os.path.join(str(tmp_path / f"planes_{tag}_{name}"), RUN_ID) for tag in ("with", "plain"))
        assert sorted(os.listdir(with_flag)) == sorted(os.listdir(without)) and len(os.listdir(without)) == 2 * NCAMS + 1
        for f in os.listdir(without):
            assert open(os.path.join(with_flag, f), "rb").read() == open(os.path.join(without, f), "rb").read(), (name, f)
    rd, _ = make_field_run(str(tmp_path / "tiny"), w=135, h=200)
    r, report, text, arrays = field_cli(["-d", os.path.dirname(rd), "-r", RUN_ID], str(tmp_path / "tiny_out"), "--survey-gpu")
    assert r.returncode != 0 and "needs frames of at least 136x136, the run's are 135x200" in r.stderr and report is None and text is None
