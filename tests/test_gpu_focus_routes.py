"""abub3hs --survey --survey-gpu --survey-focus / Run.survey(device=0, focus=...) against the host route and against the numpy
restatement (tests/focusref.py), on the run of tests/test_focus_abi.py from every source form: the same focus.txt and .npy
files, byte for byte, and the survey's report as it is without the flag; with each opt-in decoder knob; in batches of 7 and
of 1; with and without the planes, the shift file, the field and the light; the counters that show that the kernel summed
the frames; a width outside the decoders' gate."""
import os

import pytest

from autobub3hs_amd import host
from test_focus_abi import (F, H, NEV, SOFT, TOTAL, UNEVEN, W, expected_focus, focus_cli, half_trained, make_focus_run, read_focus,  # noqa: F401
                            same_focus, soft)
from test_survey_abi import NCAMS, RUN_ID, Sources, survey_cli, trained_models

pytestmark = pytest.mark.gpu

KNOBS = ("ABUB_GPU_BMP", "ABUB_GPU_UNZIP", "ABUB_GPU_PNG_TYPES", "ABUB_GPU_PNG_ADAM7", "ABUB_GPU_DECODE", "ABUB_SURVEY_BATCH",
         "ABUB_FIELD_CHUNK")
FILES = sorted(["focus.txt"] + [f"cam{c}_focus{s}.npy" for c in range(NCAMS) for s in ("", "_model")])


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def want(soft):  # noqa: F811
    src, frames = soft
    text, arrays, marr, models = expected_focus(src.rd, frames)
    assert all(m is not None for m in models)
    return text, arrays, marr


def survey(src, name, tmp_path, device=None, **kw):
    """-> (stats, report, (focus.txt, the arrays, the models' arrays), the files' bytes)"""
    out = str(tmp_path / f"{name}_{device}_{len(kw)}_focus")
    run = src.open(name) if isinstance(name, str) else name
    try:
        res, text = run.survey(nthreads=4, ncams=NCAMS, device=device, focus=out, **kw)
    finally:
        run.close()
    files = {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}
    return res, text, read_focus(out), files


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def same(got, want):  # noqa: F811
    return same_focus(got[2], want)


def test_the_trained_models_see_the_blur(want):
    """with the models the Trainer made: the saturated frame is blind, every other frame has both cells rated, and the two
    blurred frames have the lowest agreement of their camera"""
    rows = [l.split("\t") for l in want[0].splitlines()[3:3 + TOTAL]]
    ok = [r for r in rows if r[4] == "ok"]
    assert len(ok) == TOTAL - 1 and sum(r[15] == "blind" for r in ok) == 1
    assert all(r[6:8] == ["2", "0"] for r in ok if r[15] != "blind")
    keep = sorted((int(r[11]), r[3]) for r in ok if r[15] != "blind" and r[1] == "0")
    assert [k[1] for k in keep[:2]] == [SOFT[2], UNEVEN[2]] and keep[1][0] < 900 < 980 < keep[2][0]
    by_name = {(r[0], r[1], r[3]): r for r in ok}
    assert by_name[(str(SOFT[0]), "0", SOFT[2])][8:11] == ["2", "2", "0"] and by_name[(str(SOFT[0]), "0", SOFT[2])][15] == "soft"


def test_device_route_writes_the_host_routes_bytes(soft, want, tmp_path, monkeypatch):  # noqa: F811
    set_env(monkeypatch, {})
    src, frames = soft
    for name in src.cli:
        run = src.open(name)
        try:
            plain = run.survey(nthreads=4, ncams=NCAMS, device=0)[1]
        finally:
            run.close()
        cpu = survey(src, name, tmp_path)
        gpu = survey(src, name, tmp_path, device=0)
        assert same(cpu, want) and same(gpu, want), name
        assert cpu[3] == gpu[3] and sorted(gpu[3]) == FILES, name
        assert cpu[1] == gpu[1] == plain, name
        assert cpu[0]["focus_frames_kernel"] == 0 and cpu[0]["focus_frames_host"] == TOTAL - 1 and cpu[0]["focus_launches"] == 0
        assert gpu[0]["focus_frames_kernel"] + gpu[0]["focus_frames_host"] == TOTAL - 1 and gpu[0]["batches"] == 1
        assert gpu[0]["focus_frames_kernel"] == gpu[0]["frames_kernel"] == TOTAL - 1 and gpu[0]["focus_launches"] == 1
        assert gpu[0]["focus_s"] > 0 and cpu[0]["focus_host_s"] > 0
    for radius in (1, 8):
        exp = expected_focus(src.rd, frames, radius)
        got = survey(src, "dir", tmp_path, device=0, field_radius=radius)
        assert same(got, exp), radius
        assert survey(src, "packed", tmp_path, field_radius=radius)[3] == got[3], radius


def test_with_and_without_the_other_four_outputs(soft, want, tmp_path, monkeypatch):  # noqa: F811
    """the other outputs neither change the focus files nor are changed by them, on the device route"""
    set_env(monkeypatch, {})
    src, _ = soft
    alone = survey(src, "dir", tmp_path, device=0)
    for name in ("dir", "packed"):
        others = lambda tag: dict(planes=str(tmp_path / f"planes_{tag}_{name}"), shift=str(tmp_path / f"shift_{tag}_{name}.txt"),  # noqa: E731
                                  field=str(tmp_path / f"field_{tag}_{name}"), light=str(tmp_path / f"light_{tag}_{name}"))
        both = survey(src, name, tmp_path, device=0, **others("with"))
        assert same(both, want) and both[3] == alone[3], name
        res = both[0]
        assert res["focus_frames_kernel"] == res["light_frames_kernel"] == res["field_frames_kernel"] == res["shift_frames_kernel"] == TOTAL - 1
        assert res["focus_launches"] == res["light_launches"] == res["field_launches"] == res["shift_launches"] == 1
        run = src.open(name)
        try:
            run.survey(nthreads=4, ncams=NCAMS, device=0, **others("plain"))
        finally:
            run.close()
        assert open(others("with")["shift"]).read() == open(others("plain")["shift"]).read()
        for kind in ("planes", "field", "light"):
            a, b = others("with")[kind], others("plain")[kind]
            assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and os.listdir(b)
            for f in os.listdir(b):
                assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), (name, kind, f)


def test_the_kernel_sums_every_frame_with_a_model(half_trained, tmp_path, monkeypatch):  # noqa: F811
    """camera 0 does not train: its rows have no record on either route, and the kernel's counter is camera 1's ok frames"""
    set_env(monkeypatch, {})
    rd, frames = half_trained
    exp = expected_focus(rd, frames)
    assert exp[3][0] is None and exp[3][1] is not None
    for device in (None, 0):
        got = survey(None, host.Run("raw", rd + "/", "Images"), tmp_path, device=device)
        assert same(got, exp) and sorted(got[3]) == ["cam1_focus.npy", "cam1_focus_model.npy", "focus.txt"]
        assert got[0]["focus_frames_kernel" if device == 0 else "focus_frames_host"] == F * NEV - 1
        assert got[0]["focus_frames_host" if device == 0 else "focus_frames_kernel"] == 0


def test_all_five_products_on_one_job_list(half_trained, tmp_path, monkeypatch):  # noqa: F811
    """All five products at once where camera 0 has no model, so that the list of the jobs with a model is shorter than the
    batch's: in batches of one row (a batch of camera 0 has no such job and makes no launch), then in batches of 7 with the
    field's leg split job by job.  Every file is the host route's, byte for byte; each product's kernel made camera 1's ok
    rows, and the field counts one launch per chunk."""
    rd, frames = half_trained
    models = trained_models(rd, W, H)
    assert models[0] is None and models[1] is not None
    keys = sorted(frames)  # (survey order: event, camera, name)
    has_job = [frames[k] is not None and models[k[1]] is not None for k in keys]
    assert sum(has_job) == F * NEV - 1
    products = ("shift", "field", "light", "focus")

    def all_five(tag, device):
        out = {k: str(tmp_path / f"{k}_{tag}") for k in ("planes", "field", "light", "focus")}
        run = host.Run("raw", rd + "/", "Images")
        try:
            res, text = run.survey(str(tmp_path / f"report_{tag}.txt"), nthreads=4, ncams=NCAMS, device=device,
                                   shift=str(tmp_path / f"shift_{tag}.txt"), **out)
        finally:
            run.close()
        files = {f"{k}/{f}": open(os.path.join(d, f), "rb").read() for k, d in out.items() for f in sorted(os.listdir(d))}
        for k in ("report", "shift"):
            files[k] = open(str(tmp_path / f"{k}_{tag}.txt"), "rb").read()
        return res, text, files

    set_env(monkeypatch, {})
    cpu = all_five("cpu", None)
    assert all(cpu[0][f"{k}_frames_host"] == sum(has_job) and cpu[0][f"{k}_launches"] == 0 for k in products)
    assert {"field/field.txt", "light/cam1_light_model.npy", "focus/cam1_focus.npy", "planes/activity.txt"} <= set(cpu[2])
    for tag, env, batch, chunk in (("b1", {"ABUB_SURVEY_BATCH": "1"}, 1, None),
                                   ("b7", {"ABUB_SURVEY_BATCH": "7", "ABUB_FIELD_CHUNK": "1"}, 7, 1)):
        set_env(monkeypatch, env)
        res, text, files = all_five(tag, 0)
        assert text == cpu[1] and sorted(files) == sorted(cpu[2]), tag
        assert all(files[f] == cpu[2][f] for f in files), [f for f in files if files[f] != cpu[2][f]]
        per_batch = [sum(has_job[i:i + batch]) for i in range(0, TOTAL, batch)]
        assert res["device"] == 0 and res["batches"] == len(per_batch), tag
        for k in products:
            assert res[f"{k}_frames_kernel"] == sum(has_job) and res[f"{k}_frames_host"] == 0, (tag, k)
        assert res["shift_launches"] == res["light_launches"] == res["focus_launches"] == sum(n > 0 for n in per_batch), tag
        assert res["field_launches"] == (sum(per_batch) if chunk else sum(n > 0 for n in per_batch)), tag


def test_each_decoder_knob_gives_the_same_bytes(soft, want, tmp_path, monkeypatch):  # noqa: F811
    src, _ = soft
    for env, name in (({"ABUB_GPU_BMP": "1"}, "bmp"), ({"ABUB_GPU_UNZIP": "1"}, "deflated"), ({"ABUB_GPU_PNG_TYPES": "1"}, "dir"),
                      ({"ABUB_GPU_PNG_ADAM7": "1"}, "dir"), ({"ABUB_GPU_DECODE": "0"}, "dir"), ({"ABUB_GPU_DECODE": "0"}, "packed")):
        set_env(monkeypatch, env)
        got = survey(src, name, tmp_path, device=0)
        assert same(got, want), (env, name)
        assert got[0]["focus_frames_kernel"] + got[0]["focus_frames_host"] == TOTAL - 1


def test_small_batches_give_the_same_bytes(soft, want, tmp_path, monkeypatch):  # noqa: F811
    src, _ = soft
    for name in ("dir", "deflated", "packed"):
        set_env(monkeypatch, {"ABUB_SURVEY_BATCH": "7"})
        got = survey(src, name, tmp_path, device=0)
        assert same(got, want) and got[0]["batches"] == (TOTAL + 6) // 7, name
        assert got[0]["focus_launches"] == got[0]["batches"], name
        set_env(monkeypatch, {"ABUB_SURVEY_BATCH": "1"})
        got = survey(src, name, tmp_path, device=0)
        assert same(got, want) and got[0]["batches"] == TOTAL, name
        assert got[0]["focus_launches"] == TOTAL - 1 == got[0]["focus_frames_kernel"], name  # (the truncated file has no job)
    set_env(monkeypatch, {"ABUB_SURVEY_BATCH": "7"})
    got = survey(src, "packed", tmp_path, device=0, field=str(tmp_path / "f7"), shift=str(tmp_path / "s7.txt"), planes=str(tmp_path / "p7"),
                 light=str(tmp_path / "l7"))
    assert same(got, want) and got[0]["focus_launches"] == got[0]["batches"]


def test_the_kernels_counter_on_clean_runs(tmp_path, monkeypatch):
    """a run without damage, from PNG files and from its packed copy: every frame has a model and is the kernel's"""
    set_env(monkeypatch, {})
    root = str(tmp_path / "clean")
    rd, frames = make_focus_run(os.path.join(root, "data"), w=W + 4)  # (another width: plain frames, no file is truncated)
    src = Sources(root, rd)
    exp = expected_focus(rd, frames, w=W + 4)
    assert all(m is not None for m in exp[3])
    for name in ("dir", "packed"):
        got = survey(src, name, tmp_path, device=0)
        assert same(got, exp) and got[0]["rc"] == 0
        assert got[0]["focus_frames_kernel"] == got[0]["frames_kernel"] == TOTAL and got[0]["focus_frames_host"] == 0
        assert got[0]["host_decoded"] == 0
        assert f"run frames {TOTAL} blind 0 " in got[2][0]


def test_a_width_outside_the_gate_takes_the_host_route_whole(tmp_path, monkeypatch):
    """138 columns (no multiple of 4: no GPU decoder takes the width): the run goes to the host whole, and the files are the
    host route's"""
    set_env(monkeypatch, {})
    rd, frames = make_focus_run(str(tmp_path / "data"), w=138, h=140)
    exp = expected_focus(rd, frames, w=138, h=140)
    assert all(m is not None for m in exp[3])
    got = survey(None, host.Run("raw", rd + "/", "Images"), tmp_path, device=0)
    assert same(got, exp) and got[0]["rc"] == 0
    assert got[0]["device"] == -1 and got[0]["focus_frames_kernel"] == 0 and got[0]["focus_launches"] == 0
    assert got[0]["focus_frames_host"] == TOTAL


def test_a_42_wide_run_is_refused_on_both_routes(tmp_path, monkeypatch):
    """42 columns hold no whole cell: the refusal comes before the route is chosen, the same with and without a device; a
    survey without the focus still runs, on the host"""
    set_env(monkeypatch, {})
    rd, frames = make_focus_run(str(tmp_path / "data"), w=42, h=140)
    for device in (None, 0):
        run = host.Run("raw", rd + "/", "Images")
        try:
            with pytest.raises(RuntimeError, match="need frames of at least 136x136, the run's are 42x140"):
                run.survey(nthreads=4, ncams=NCAMS, device=device, focus=str(tmp_path / "o"))
            res, _ = run.survey(nthreads=4, ncams=NCAMS, device=device)
        finally:
            run.close()
        assert res["device"] == -1 and not os.path.exists(str(tmp_path / "o"))


def test_cli_on_the_device_route(soft, want, tmp_path):  # noqa: F811
    src, _ = soft
    for name in ("dir", "stored", "packed"):
        others = lambda tag: ["--survey-gpu", "--survey-planes", str(tmp_path / f"planes_{tag}_{name}"), "--survey-shift",  # noqa: E731
                              str(tmp_path / f"shift_{tag}_{name}.txt"), "--survey-field", str(tmp_path / f"field_{tag}_{name}"),
                              "--survey-light", str(tmp_path / f"light_{tag}_{name}")]
        plain, report_plain = survey_cli(src.cli[name], str(tmp_path / f"plain_{name}.txt"), *others("plain"))
        a = focus_cli(src.cli[name], str(tmp_path / f"a_{name}"), "--survey-gpu")
        b = focus_cli(src.cli[name], str(tmp_path / f"b_{name}"), *others("with"))
        assert a[0].returncode == b[0].returncode == plain.returncode == 1, a[0].stderr + b[0].stderr
        assert same(a, want) and same(b, want), name
        assert a[1] == b[1] == report_plain, name
        line = [l for l in b[0].stdout.splitlines() if l.startswith("survey-focus: ")]
        assert len(line) == 1 and f"radius 4, {TOTAL - 1} frames summed on the GPU in 1 launches, 0 on the host" in line[0], b[0].stdout
        assert open(str(tmp_path / f"shift_with_{name}.txt")).read() == open(str(tmp_path / f"shift_plain_{name}.txt")).read()
        for kind in ("planes", "field", "light"):
            with_flag, without = (os.path.join(str(tmp_path / f"{kind}_{tag}_{name}"), RUN_ID) for tag in ("with", "plain"))
            assert sorted(os.listdir(with_flag)) == sorted(os.listdir(without)) and os.listdir(without)
            for f in os.listdir(without):
                assert open(os.path.join(with_flag, f), "rb").read() == open(os.path.join(without, f), "rb").read(), (name, f)
