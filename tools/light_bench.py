#!/usr/bin/env python3
"""abub_frame_light_cells_dev and abub3hs --survey --survey-light [--survey-gpu] measured on one GPU box, in one call ->
profiles/r24/light.json.  Set and protocol are those of tools/field_bench.py (its frames, its model, device events, windows
alternating in one call).
  (a) kernel: 1024 resident 1280x1024 synth frames in 25 stacks with a model, every frame against mu on the grid of R = 4
      (9 x 7 cells); three launches per window, five windows alternating with abub_frame_shift_cells_dev at R = 1 and with
      abub_frame_stats_dev on the same frames; ms per launch (median and range), frames per second, and the implied rate
      against the bytes of p and m inside the cells (2 * cells * 16384 per frame; mu is one plane that every frame reads
      again, so most likely from a cache: the rate is no fraction of the HBM bandwidth); some records are checked against
      lightCellsHost first;
  (c) end to end: the 1025-frame run of survey_bench part (c), as PNG files and repacked, surveyed by the CLI on the host
      route and with --survey-gpu, with --survey-light and without, each three times alternating, from the page cache;
      medians of the CLI's own seconds; the light's files and the reports compared byte for byte;
  (d) parent comparison: bench.py --steps 20 --warmup 5, parent build and this tree in the balanced twelve-run order of
      tools/verify_bench.py, dumped outputs compared byte for byte;
  (e) the committed sample frame of the 40l-19 data (tests/golden) as a three-frame event whose third frame is scaled to
      0.95 on the host ((p * 95 + 50) / 100): light.txt of both routes.
usage: python3 tools/light_bench.py [--parts acde] [--parent PARENT_CHECKOUT] [--balanced [ORDER]] [--out profiles/r24/light.json]
                                    [--frames 1024]"""
import argparse, io, json, os, shutil, statistics, subprocess, sys, tempfile, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from survey_bench import F, H, P, W, model_of, part_d, stacks  # noqa: E402

R = 4


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
    d_s6 = torch.from_numpy(s6.reshape(-1)).to(dev)
    jobs = np.array([[i * P, 0] for i in range(n)], dtype=np.int64)
    ncx, ncy, x0, y0 = hip.field_grid(W, H, R)
    cells = ncx * ncy
    status, rec = hip.frame_light_cells(slab, d_mu, jobs, W, H, x0, y0, ncx, ncy)
    assert not status.any()
    for i in (0, F - 1, n - 1):
        assert np.array_equal(rec[i], host.light_cells_host(fr[i][2], mu, x0, y0, ncx, ncy)), i
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    d_jobs = torch.from_numpy(jobs).to(dev)
    d_sjobs = torch.from_numpy(np.array([[i * P, -1, 0] for i in range(n)], dtype=np.int64)).to(dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    lrec = torch.empty((n * cells * 6,), dtype=torch.int32, device=dev)
    c1 = hip.field_grid(W, H, 1)
    csurf = torch.empty((n * c1[0] * c1[1] * 9,), dtype=torch.int32, device=dev)
    sres = torch.empty((n * 64,), dtype=torch.uint8, device=dev)

    def light(rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_light_cells_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_mu.numel(), d_jobs.data_ptr(), n, W,
                                                    H, x0, y0, ncx, ncy, status.data_ptr(), lrec.data_ptr(), stream), "light")

    def field(rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_shift_cells_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_mu.numel(), d_jobs.data_ptr(), n, W,
                                                    H, 1, status.data_ptr(), csurf.data_ptr(), stream), "cells")

    def stats(rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_stats_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_s6.data_ptr(), d_mu.numel(),
                                              d_sjobs.data_ptr(), n, P, sres.data_ptr(), stream), "stats")

    def timed(fn, rep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(rep)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / rep

    kernels = {"light": light, "field_R1": field, "stats": stats}
    for fn in kernels.values():
        fn(1)
    torch.cuda.synchronize()
    t = {k: [] for k in kernels}
    for _ in range(5):
        for k, fn in kernels.items():
            t[k].append(timed(fn, 3))
    med = {k: statistics.median(v) for k, v in t.items()}
    bytes_in_cells = 2 * cells * 16384
    return {"frames": n, "W": W, "H": H, "grid": [ncx, ncy, x0, y0], "cells": cells, "field_R1_cells": c1[0] * c1[1],
            "launches_per_window": 3, "windows": 5, "ms_per_launch": t, "ms_per_launch_median": med,
            "ms_per_launch_range": {k: [min(v), max(v)] for k, v in t.items()}, "frames_per_s": n / med["light"] * 1e3,
            "bytes_of_p_and_m_in_the_cells_per_frame": bytes_in_cells,
            "implied_GB_per_s": bytes_in_cells * n / med["light"] * 1e3 / 1e9,
            "implied_rate_note": "mu is one plane read again by every frame, most likely from a cache: not an HBM fraction",
            "light_over_field_R1_time": med["light"] / med["field_R1"], "light_over_stats_time": med["light"] / med["stats"]}


def part_c(n):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image

    run_id = "20200925_0"
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="1", ABUB_THREADS="16")
    tmp = tempfile.mkdtemp(prefix="abub_light_")
    try:
        n = (n + F - 1) // F * F
        fr = stacks(n)

        def write(job):
            s, k, f = job
            b = io.BytesIO()
            Image.fromarray(f).save(b, format="PNG", compress_level=1)
            os.makedirs(os.path.join(tmp, "png", run_id, str(s), "Images"), exist_ok=True)
            open(os.path.join(tmp, "png", run_id, str(s), "Images", f"cam0_image{30 + k}.png"), "wb").write(b.getvalue())

        with ThreadPoolExecutor(16) as ex:
            list(ex.map(write, fr))
        with open(os.path.join(tmp, "png", run_id, run_id + ".txt"), "w") as f:
            for s in range((n + F - 1) // F):
                f.write(f"{run_id} {s} a b c d e f g h i\n")
        r = subprocess.run([exe, "-d", os.path.join(tmp, "png"), "-r", run_id, "--repack", os.path.join(tmp, "packed"), "--repack-gpu"],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out, reports, lights = {}, set(), set()
        configs = [(route, with_light) for with_light in (True, False) for route in ("host", "gpu")]
        for kind in ("png", "packed"):
            series = {f"{route}{'_light' if fl else ''}": [] for route, fl in configs}
            lines = {}
            for rep in range(3):
                for route, fl in configs:
                    key = f"{route}{'_light' if fl else ''}"
                    rep_file, light_dir = os.path.join(tmp, f"{kind}_{key}.txt"), os.path.join(tmp, f"{kind}_{key}_light")
                    args = [exe, "-d", os.path.join(tmp, kind), "-r", run_id, "--survey", rep_file]
                    args += ["--survey-light", light_dir] if fl else []
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
                        d = os.path.join(light_dir, run_id)
                        lights.add(tuple(open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))))
            med = {k: statistics.median(x["survey_s"] for x in v) for k, v in series.items()}
            out[kind] = {"runs": series, "survey_s_median": med, "frames_per_s": {k: n / v for k, v in med.items()},
                         "gpu_over_host_with_light": med["host_light"] / med["gpu_light"], "gpu_over_host_without": med["host"] / med["gpu"],
                         "light_adds_s": {"host": med["host_light"] - med["host"], "gpu": med["gpu_light"] - med["gpu"]}, "last_lines": lines}
        out["reports_identical"] = len(reports) == 1
        out["light_files_identical"] = len(lights) == 1
        out["frames"] = n
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def part_e():
    from PIL import Image

    run_id = "20200925_0"
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    sample = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "sample_40l19_cam1_image30.png")).convert("L"))
    h, w = sample.shape
    dimmed = ((sample.astype(np.int64) * 95 + 50) // 100).astype(np.uint8)
    tmp = tempfile.mkdtemp(prefix="abub_light_sample_")
    try:
        d = os.path.join(tmp, run_id, "0", "Images")
        os.makedirs(d)
        for k, img in enumerate((sample, sample, dimmed)):
            Image.fromarray(img).save(os.path.join(d, f"cam1_image{30 + k}.png"))
        texts, shifts, fields = [], [], []
        for flag in ([], ["--survey-gpu"]):
            rep, sh, fd, ld = (os.path.join(tmp, f) for f in ("report.txt", "shift.txt", "field", "light"))
            r = subprocess.run([exe, "-d", tmp, "-r", run_id, "-D", "40l-19", "--survey", rep, "--survey-shift", sh, "--survey-field", fd,
                                "--survey-light", ld] + flag,
                               env=dict(os.environ, ABUB_NUM_CAMS="2"), capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            texts.append(open(os.path.join(ld, run_id, "light.txt")).read())
            shifts.append(open(sh).read())
            fields.append(open(os.path.join(fd, run_id, "field.txt")).read())
        assert texts[0] == texts[1] and shifts[0] == shifts[1] and fields[0] == fields[1]
        return {"frames": 3, "W": int(w), "H": int(h), "third_frame": "(p * 95 + 50) / 100", "routes_identical": True,
                "light_txt": texts[0].splitlines(), "shift_file": shifts[0].splitlines(),
                "field_txt_rows": [l for l in fields[0].splitlines() if l.startswith("0\t")]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="acde")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "light.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--balanced", nargs="?", const="TPPTTPPTTPPT", default="TPPTTPPTTPPT")
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):  # (a call that measures some of the parts keeps the others)
        result = json.load(open(a.out))
    for part, fn in (("a", lambda: part_a(a.frames)), ("c", lambda: part_c(a.frames)), ("e", part_e),
                     ("d", lambda: part_d(a.parent, a.balanced))):
        key = {"a": "kernel", "c": "end_to_end", "d": "parent_comparison_" + a.balanced, "e": "sample_frame_run"}[part]
        if part not in a.parts or (part == "d" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
