"""abub3hs --survey --survey-gpu --survey-lines / Run.survey(device=0, lines=...) against the host route and against the numpy
restatement (tests/linesref.py), on the run of tests/test_lines_abi.py (two cameras, one untrained; a band of rows and a stripe
of columns up by 3 levels, a torn and a repeated frame, an undecodable, a missing and a wider frame) from a directory, a stored
archive and a repacked copy: the same lines.txt and .npy files, byte for byte, and the survey's report as it is without the
flag; together with every other product in one call; in small batches, whose boundaries fall inside a stack and inside the
torn frame's pairing; in calls of a few jobs (the field's chunking knob); the kinds as planted; the CLI."""
import os
import subprocess

import pytest

from autobub3hs_amd import host
from test_lines_abi import (F, H, RECORDS, TORN, TOTAL, UNTRAINED, W, check_kinds, expected_lines, make_lines_run, read_lines, same_lines)
from test_survey_abi import ENV, EXE, NCAMS, RUN_ID, Sources

pytestmark = pytest.mark.gpu

KNOBS = ("ABUB_GPU_BMP", "ABUB_GPU_UNZIP", "ABUB_GPU_PNG_TYPES", "ABUB_GPU_PNG_ADAM7", "ABUB_GPU_DECODE", "ABUB_SURVEY_BATCH",
         "ABUB_FIELD_CHUNK")
FILES = ["cam1_lines_cols.npy", "cam1_lines_model_cols.npy", "cam1_lines_model_rows.npy", "cam1_lines_rows.npy", "lines.txt"]
FORMS = ("dir", "stored", "packed")
WK = W + 1  # 268: the run one column wider, a width the GPU decoders take (a multiple of 4), so that the kernel sums it


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    """the run at 268 x 137: the device route takes it"""
    root = str(tmp_path_factory.mktemp("lines_routes"))
    rd, frames = make_lines_run(os.path.join(root, "data"), w=WK)
    return Sources(root, rd), frames


@pytest.fixture(scope="module")
def want(planted):
    src, frames = planted
    text, arrays, marr, models = expected_lines(src.rd, frames, w=WK)
    assert models[UNTRAINED] is None and models[1] is not None
    return text, arrays, marr


@pytest.fixture(scope="module")
def odd(tmp_path_factory):
    """the run at 267 x 137: no GPU decoder takes an odd width, so the device route hands it to the host whole"""
    root = str(tmp_path_factory.mktemp("lines_routes_odd"))
    rd, frames = make_lines_run(os.path.join(root, "data"))
    return Sources(root, rd), frames


def survey(src, name, tmp_path, device=None, **kw):
    """-> (stats, report, (lines.txt, the arrays, the models' arrays), the files' bytes)"""
    out = str(tmp_path / f"{name}_{device}_{len(kw)}_lines")
    run = src.open(name)
    try:
        res, text = run.survey(nthreads=4, ncams=NCAMS, device=device, lines=out, **kw)
    finally:
        run.close()
    return res, text, read_lines(out), {f: open(os.path.join(out, f), "rb").read() for f in sorted(os.listdir(out))}


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def counters(res):
    return res["lines_frames_kernel"], res["lines_frames_host"], res["lines_launches"]


def test_the_kinds_come_out_as_planted_with_the_trained_model(want):
    """with the model the Trainer made: every untouched frame is steady, the band's frames banded, the stripe's striped, the
    torn frame torn from row 60 on, the copied frame repeated; what tests/test_lines_abi.py shows for the restatement's own
    model"""
    check_kinds(*want, w=WK)


def test_the_odd_width_falls_back_whole_with_the_same_bytes(odd, tmp_path, monkeypatch):
    """267 columns: from every form --survey-gpu writes the host route's bytes, which are the restatement's, the kinds come out
    as planted, and the counters say that the host summed the run"""
    set_env(monkeypatch, {})
    src, frames = odd
    exp = expected_lines(src.rd, frames)
    assert exp[3][UNTRAINED] is None and exp[3][1] is not None and (W, H) == (267, 137)
    check_kinds(*exp[:3])
    for name in FORMS:
        cpu = survey(src, name, tmp_path)
        gpu = survey(src, name, tmp_path, device=0)
        assert same_lines(cpu[2], exp) and same_lines(gpu[2], exp) and cpu[3] == gpu[3] and cpu[1] == gpu[1], name
        assert gpu[0]["device"] == -1 and counters(gpu[0]) == (0, RECORDS, 0)


def test_device_route_writes_the_host_routes_bytes(planted, want, tmp_path, monkeypatch):
    set_env(monkeypatch, {})
    src, _ = planted
    for name in FORMS:
        run = src.open(name)
        try:
            plain = run.survey(nthreads=4, ncams=NCAMS, device=0)[1]
        finally:
            run.close()
        cpu = survey(src, name, tmp_path)
        gpu = survey(src, name, tmp_path, device=0)
        assert same_lines(cpu[2], want) and same_lines(gpu[2], want), name
        assert cpu[3] == gpu[3] and sorted(gpu[3]) == FILES, name
        assert cpu[1] == gpu[1] == plain, name
        # the kernel sums every ok row of the camera with a model; the wider and the undecodable row are the host's, without a record
        assert counters(cpu[0]) == (0, RECORDS, 0) and counters(gpu[0]) == (RECORDS, 0, 1), name
        assert gpu[0]["batches"] == 1 and gpu[0]["frames_host_route"] >= 3


def test_together_with_every_other_product_in_one_call(planted, want, tmp_path, monkeypatch):
    """field, light, focus, noise, planes and shift in the same call: every file of every product equals its single-product
    call's"""
    set_env(monkeypatch, {})
    src, _ = planted
    for name in ("dir", "packed"):
        at = lambda tag, kind: str(tmp_path / f"{kind}_{tag}_{name}")  # noqa: E731
        alone = survey(src, name, tmp_path, device=0)
        both = survey(src, name, tmp_path, device=0, **{k: at("all", k) for k in ("field", "light", "focus", "noise", "planes")},
                      shift=at("all", "shift") + ".txt")
        assert same_lines(both[2], want) and both[3] == alone[3] and both[1] == alone[1], name
        res = both[0]
        assert counters(res) == (RECORDS, 0, 1)
        assert res["light_frames_kernel"] == res["field_frames_kernel"] == res["focus_frames_kernel"] == res["shift_frames_kernel"] == RECORDS
        for kind in ("field", "light", "focus", "noise", "planes", "shift"):
            run = src.open(name)
            try:
                run.survey(nthreads=4, ncams=NCAMS, device=0, **{kind: at("one", kind) + (".txt" if kind == "shift" else "")})
            finally:
                run.close()
            if kind == "shift":
                assert open(at("all", kind) + ".txt", "rb").read() == open(at("one", kind) + ".txt", "rb").read(), name
                continue
            a, b = at("all", kind), at("one", kind)
            assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and os.listdir(b)
            for f in os.listdir(b):
                assert open(os.path.join(a, f), "rb").read() == open(os.path.join(b, f), "rb").read(), (name, kind, f)


def test_small_batches_and_small_calls(planted, want, tmp_path, monkeypatch):
    """batches of 7 begin inside a stack of 8, and one begins between the torn frame (row 29 of the survey) and the frame it
    is paired with (row 27): the reference frames lie in the batch before and are read again; batches of 1: every reference
    frame is.  ABUB_FIELD_CHUNK: the launches are of at most so many jobs, and nothing else changes"""
    src, _ = planted
    e, c, k = TORN
    first = (e * NCAMS + c) * F
    assert (first + k - 2) // 7 != (first + k) // 7 and first % 7
    for name, batch in (("dir", 7), ("packed", 7), ("stored", 1)):
        set_env(monkeypatch, {"ABUB_SURVEY_BATCH": str(batch)})
        got = survey(src, name, tmp_path, device=0)
        assert same_lines(got[2], want) and got[0]["batches"] == (TOTAL + batch - 1) // batch, (name, batch)
        assert counters(got[0])[:2] == (RECORDS, 0) and got[0]["reread"] > 0, (name, batch)
    set_env(monkeypatch, {"ABUB_FIELD_CHUNK": "5"})
    got = survey(src, "dir", tmp_path, device=0, field=str(tmp_path / "f5"))
    assert same_lines(got[2], want) and counters(got[0]) == (RECORDS, 0, (RECORDS + 4) // 5) and got[0]["field_launches"] == (RECORDS + 4) // 5
    set_env(monkeypatch, {"ABUB_SURVEY_BATCH": "7", "ABUB_FIELD_CHUNK": "2"})
    got = survey(src, "packed", tmp_path, device=0, noise=str(tmp_path / "n7"), planes=str(tmp_path / "p7"))
    assert same_lines(got[2], want) and counters(got[0])[:2] == (RECORDS, 0) and counters(got[0])[2] > RECORDS // 2


def test_cli_on_the_device_route(planted, want, tmp_path):
    src, _ = planted

    def lines_cli(name, stem, *more):
        r = subprocess.run([EXE] + src.cli[name] + ["--survey", stem + ".txt", "--survey-lines", stem + "_lines", *more], env=ENV,
                           capture_output=True, text=True, timeout=120)
        return r, open(stem + ".txt").read(), read_lines(os.path.join(stem + "_lines", RUN_ID))

    for name in FORMS:
        host_route = lines_cli(name, str(tmp_path / f"h_{name}"))
        gpu = lines_cli(name, str(tmp_path / f"g_{name}"), "--survey-gpu")
        assert host_route[0].returncode == gpu[0].returncode == 1, host_route[0].stderr + gpu[0].stderr  # (the damaged files)
        assert same_lines(host_route[2], want) and same_lines(gpu[2], want) and host_route[1] == gpu[1], name
        line = [l for l in gpu[0].stdout.splitlines() if l.startswith("survey-lines: ")]
        assert len(line) == 1 and f"{RECORDS} frames summed on the GPU in 1 launches, 0 on the host" in line[0], gpu[0].stdout
        assert " torn 1 " in gpu[2][0].splitlines()[-1] and " repeated 1 " in gpu[2][0].splitlines()[-1]
