#!/usr/bin/env python3
"""abub_frame_focus_cells_dev and abub3hs --survey --survey-focus [--survey-gpu] measured on one GPU box, in one call ->
profiles/r25/focus.json.  Set and protocol are those of tools/light_bench.py (its frames, its model, device events, windows
alternating in one call).
  (a) kernel: 1024 resident 1280x1024 synth frames in 25 stacks with a model, every frame against mu on the grid of R = 4
      (9 x 7 cells); three launches per window, five windows alternating with abub_frame_light_cells_dev on the same grid and
      with abub_frame_shift_cells_dev at R = 1 on the same frames; ms per launch (median and range), frames per second, the
      ratios to the two yardsticks; some records are checked against focusCellsHost first;
  (c) end to end: the 1025-frame run of survey_bench part (c), as PNG files and repacked, surveyed by the CLI on the host
      route and with --survey-gpu, with --survey-focus and without, each three times alternating, from the page cache;
      medians of the CLI's own seconds; the focus files and the reports compared byte for byte;
  (s) a steady run: one synth scene under rounded normal noise (sigma 1.5 grey levels), 12 events of 10 frames, trained by the
      project's Trainer and surveyed with --survey-gpu --survey-focus: how many rated cells come out `changed` although
      nothing changed (the training-noise bias of DESIGN's limits), and the range of their keep;
  (d) parent comparison: bench.py --steps 20 --warmup 5, parent build and this tree in the balanced twelve-run order of
      tools/verify_bench.py, dumped outputs compared byte for byte;
  (e) the committed sample frame of the 40l-19 data (tests/golden) as a three-frame event whose third frame is blurred once
      with the 3 x 3 binomial (sum + 8) / 16 on the host: focus.txt of both routes, next to the shift file, the field and
      the light of the same run.
usage: python3 tools/focus_bench.py [--parts acsde] [--parent PARENT_CHECKOUT] [--balanced [ORDER]] [--out profiles/r25/focus.json]
                                    [--frames 1024]"""
import argparse, io, json, os, shutil, statistics, subprocess, sys, tempfile, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from survey_bench import F, H, P, W, model_of, part_d, stacks  # noqa: E402

R = 4
RUN_ID = "20200925_0"
EXE = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")


def part_a(n):
    import torch
    from autobub3hs_amd import _lib, hip, host

    fr = stacks(n)
    mu, _, s6 = model_of(fr)
    dev = torch.device("cuda:0")
    slab = torch.empty((n, P), dtype=torch.uint8, device=dev)
    for i, (_, _, f) in enumerate(fr):
        slab[i] = torch.from_numpy(f.reshape(-1)).to(dev)
    slab = slab.reshape(-1)
    d_mu = torch.from_numpy(mu.reshape(-1)).to(dev)
    jobs = np.array([[i * P, 0] for i in range(n)], dtype=np.int64)
    ncx, ncy, x0, y0 = hip.field_grid(W, H, R)
    cells = ncx * ncy
    status, rec = hip.frame_focus_cells(slab, d_mu, jobs, W, H, x0, y0, ncx, ncy)
    assert not status.any()
    for i in (0, F - 1, n - 1):
        assert np.array_equal(rec[i], host.focus_cells_host(fr[i][2], mu, x0, y0, ncx, ncy)), i
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    d_jobs = torch.from_numpy(jobs).to(dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    frec = torch.empty((n * cells * 5,), dtype=torch.int32, device=dev)
    lrec = torch.empty((n * cells * 6,), dtype=torch.int32, device=dev)
    c1 = hip.field_grid(W, H, 1)
    csurf = torch.empty((n * c1[0] * c1[1] * 9,), dtype=torch.int32, device=dev)

    def focus(rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_focus_cells_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_mu.numel(), d_jobs.data_ptr(), n, W,
                                                    H, x0, y0, ncx, ncy, status.data_ptr(), frec.data_ptr(), stream), "focus")

    def light(rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_light_cells_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_mu.numel(), d_jobs.data_ptr(), n, W,
                                                    H, x0, y0, ncx, ncy, status.data_ptr(), lrec.data_ptr(), stream), "light")

    def field(rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_shift_cells_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_mu.numel(), d_jobs.data_ptr(), n, W,
                                                    H, 1, status.data_ptr(), csurf.data_ptr(), stream), "cells")

    def timed(fn, rep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(rep)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / rep

    kernels = {"focus": focus, "light": light, "field_R1": field}
    for fn in kernels.values():
        fn(1)
    torch.cuda.synchronize()
    t = {k: [] for k in kernels}
    for _ in range(5):
        for k, fn in kernels.items():
            t[k].append(timed(fn, 3))
    med = {k: statistics.median(v) for k, v in t.items()}
    bytes_in_tiles = 2 * cells * 130 * 130
    return {"frames": n, "W": W, "H": H, "grid": [ncx, ncy, x0, y0], "cells": cells, "field_R1_cells": c1[0] * c1[1],
            "launches_per_window": 3, "windows": 5, "ms_per_launch": t, "ms_per_launch_median": med,
            "ms_per_launch_range": {k: [min(v), max(v)] for k, v in t.items()}, "frames_per_s": n / med["focus"] * 1e3,
            "bytes_of_p_and_m_in_the_tiles_per_frame": bytes_in_tiles,
            "implied_GB_per_s": bytes_in_tiles * n / med["focus"] * 1e3 / 1e9,
            "implied_rate_note": "mu is one plane read again by every frame, most likely from a cache: not an HBM fraction",
            "focus_over_light_time": med["focus"] / med["light"], "focus_over_field_R1_time": med["focus"] / med["field_R1"],
            "lds_free_form": "not built"}


def write_run(root, frames, nstacks):
    """frames: [(stack, k, image)] -> the run directory tree under root, PNG files at compression level 1"""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image

    def write(job):
        s, k, f = job
        b = io.BytesIO()
        Image.fromarray(f).save(b, format="PNG", compress_level=1)
        os.makedirs(os.path.join(root, RUN_ID, str(s), "Images"), exist_ok=True)
        open(os.path.join(root, RUN_ID, str(s), "Images", f"cam0_image{30 + k}.png"), "wb").write(b.getvalue())

    with ThreadPoolExecutor(16) as ex:
        list(ex.map(write, frames))
    with open(os.path.join(root, RUN_ID, RUN_ID + ".txt"), "w") as f:
        for s in range(nstacks):
            f.write(f"{RUN_ID} {s} a b c d e f g h i\n")


def part_c(n):
    env = dict(os.environ, ABUB_NUM_CAMS="1", ABUB_THREADS="16")
    tmp = tempfile.mkdtemp(prefix="abub_focus_")
    try:
        n = (n + F - 1) // F * F
        write_run(os.path.join(tmp, "png"), stacks(n), (n + F - 1) // F)
        r = subprocess.run([EXE, "-d", os.path.join(tmp, "png"), "-r", RUN_ID, "--repack", os.path.join(tmp, "packed"), "--repack-gpu"],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out, reports, focuses = {}, set(), set()
        configs = [(route, with_focus) for with_focus in (True, False) for route in ("host", "gpu")]
        for kind in ("png", "packed"):
            series = {f"{route}{'_focus' if fl else ''}": [] for route, fl in configs}
            lines = {}
            for rep in range(3):
                for route, fl in configs:
                    key = f"{route}{'_focus' if fl else ''}"
                    rep_file, focus_dir = os.path.join(tmp, f"{kind}_{key}.txt"), os.path.join(tmp, f"{kind}_{key}_focus")
                    args = [EXE, "-d", os.path.join(tmp, kind), "-r", RUN_ID, "--survey", rep_file]
                    args += ["--survey-focus", focus_dir] if fl else []
                    args += ["--survey-gpu"] if route == "gpu" else []
                    t0 = time.perf_counter()
                    r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=1200)
                    wall = time.perf_counter() - t0
                    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
                    line = [l for l in r.stdout.splitlines() if l.startswith("survey: ")][-1]
                    series[key].append({"survey_s": float(line.rsplit("; ", 1)[1].split(" s,")[0]), "process_s": wall})
                    lines[key] = [l.replace(tmp, "TMP") for l in r.stdout.splitlines() if l.startswith("survey")]
                    reports.add(open(rep_file, "rb").read())
                    if fl:
                        d = os.path.join(focus_dir, RUN_ID)
                        focuses.add(tuple(open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))))
            med = {k: statistics.median(x["survey_s"] for x in v) for k, v in series.items()}
            out[kind] = {"runs": series, "survey_s_median": med, "frames_per_s": {k: n / v for k, v in med.items()},
                         "survey_s_range": {k: [min(x["survey_s"] for x in v), max(x["survey_s"] for x in v)] for k, v in series.items()},
                         "gpu_over_host_with_focus": med["host_focus"] / med["gpu_focus"], "gpu_over_host_without": med["host"] / med["gpu"],
                         "focus_adds_s": {"host": med["host_focus"] - med["host"], "gpu": med["gpu_focus"] - med["gpu"]}, "last_lines": lines}
        out["reports_identical"] = len(reports) == 1
        out["focus_files_identical"] = len(focuses) == 1
        out["frames"] = n
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def focus_rows(text):
    """focus.txt -> its ok rows with a record, as dicts of the header's columns"""
    lines = text.splitlines()
    names = lines[2].split("\t")
    return [dict(zip(names, l.split("\t"))) for l in lines[3:] if "\t" in l and l.split("\t")[5] != "-"]


def part_s(events=12, per=10, sigma=1.5):
    from autobub3hs_amd import synth

    scene = np.asarray(synth.render_event(W, H, synth.random_spec(W, H, F, 0, 0, p_second=0.2), 0, 0))[0].astype(np.float64)
    rs = np.random.RandomState(25)
    frames = [(s, k, np.clip(np.rint(scene + rs.normal(0, sigma, scene.shape)), 0, 255).astype(np.uint8)) for s in range(events)
              for k in range(per)]
    tmp = tempfile.mkdtemp(prefix="abub_focus_steady_")
    try:
        write_run(tmp, frames, events)
        rep, fd = os.path.join(tmp, "report.txt"), os.path.join(tmp, "focus")
        r = subprocess.run([EXE, "-d", tmp, "-r", RUN_ID, "--survey", rep, "--survey-focus", fd, "--survey-gpu"],
                           env=dict(os.environ, ABUB_NUM_CAMS="1", ABUB_THREADS="16"), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        text = open(os.path.join(fd, RUN_ID, "focus.txt")).read()
        rows = focus_rows(text)
        model = [l for l in open(rep).read().splitlines() if l.startswith("model")]
        if not rows or all(q["kind"] == "blind" for q in rows):
            return {"note": "no rated row: the camera did not train or every cell is blind", "report_model_lines": model,
                    "focus_txt_tail": text.splitlines()[3 + len(frames):]}
        return {"events": events, "frames_per_event": per, "noise_sigma": sigma, "W": W, "H": H, "frames_with_a_record": len(rows),
                "rated_cells": sum(int(q["rated"]) for q in rows), "clipped_cells": sum(int(q["clipped"]) for q in rows),
                "changed_cells": sum(int(q["changed"]) for q in rows), "softer_cells": sum(int(q["softer"]) for q in rows),
                "harder_cells": sum(int(q["harder"]) for q in rows), "kinds": {k: sum(q["kind"] == k for q in rows) for k in
                                                                              ("blind", "steady", "soft", "uneven")},
                "keep_milli_range": [min(int(q["keep_milli"]) for q in rows if q["keep_milli"] != "-"),
                                     max(int(q["keep_milli"]) for q in rows if q["keep_milli"] != "-")],
                "keep_min_lowest": min(int(q["keep_min"]) for q in rows if q["keep_min"] != "-"),
                "report_model_lines": model, "focus_txt_tail": text.splitlines()[3 + len(frames):]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def part_e():
    from PIL import Image

    sample = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "sample_40l19_cam1_image30.png")).convert("L"))
    h, w = sample.shape
    a = sample.astype(np.int64)
    soft = sample.copy()
    soft[1:-1, 1:-1] = (a[:-2, :-2] + 2 * a[:-2, 1:-1] + a[:-2, 2:] + 2 * a[1:-1, :-2] + 4 * a[1:-1, 1:-1] + 2 * a[1:-1, 2:] + a[2:, :-2]
                        + 2 * a[2:, 1:-1] + a[2:, 2:] + 8) // 16
    tmp = tempfile.mkdtemp(prefix="abub_focus_sample_")
    try:
        d = os.path.join(tmp, RUN_ID, "0", "Images")
        os.makedirs(d)
        for k, img in enumerate((sample, sample, soft)):
            Image.fromarray(img).save(os.path.join(d, f"cam1_image{30 + k}.png"))
        texts, shifts, fields, lights = [], [], [], []
        for flag in ([], ["--survey-gpu"]):
            rep, sh, fd, ld, od = (os.path.join(tmp, f) for f in ("report.txt", "shift.txt", "field", "light", "focus"))
            r = subprocess.run([EXE, "-d", tmp, "-r", RUN_ID, "-D", "40l-19", "--survey", rep, "--survey-shift", sh, "--survey-field", fd,
                                "--survey-light", ld, "--survey-focus", od] + flag,
                               env=dict(os.environ, ABUB_NUM_CAMS="2"), capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            texts.append(open(os.path.join(od, RUN_ID, "focus.txt")).read())
            shifts.append(open(sh).read())
            fields.append(open(os.path.join(fd, RUN_ID, "field.txt")).read())
            lights.append(open(os.path.join(ld, RUN_ID, "light.txt")).read())
        assert texts[0] == texts[1] and shifts[0] == shifts[1] and fields[0] == fields[1] and lights[0] == lights[1]
        return {"frames": 3, "W": int(w), "H": int(h), "third_frame": "3 x 3 binomial, (sum + 8) / 16, once", "routes_identical": True,
                "focus_txt": texts[0].splitlines(), "shift_file": shifts[0].splitlines(),
                "field_txt_rows": [l for l in fields[0].splitlines() if l.startswith("0\t")],
                "light_txt_rows": [l for l in lights[0].splitlines() if l.startswith("0\t")]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="acsde")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25", "focus.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--balanced", nargs="?", const="TPPTTPPTTPPT", default="TPPTTPPTTPPT")
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):  # (a call that measures some of the parts keeps the others)
        result = json.load(open(a.out))
    for part, fn in (("a", lambda: part_a(a.frames)), ("c", lambda: part_c(a.frames)), ("s", part_s), ("e", part_e),
                     ("d", lambda: part_d(a.parent, a.balanced))):
        key = {"a": "kernel", "c": "end_to_end", "s": "steady_run", "d": "parent_comparison_" + a.balanced, "e": "sample_frame_run"}[part]
        if part not in a.parts or (part == "d" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
