#!/usr/bin/env python3
"""abub_frame_noise_cells_dev and abub3hs --survey --survey-noise [--survey-gpu] measured on one GPU box, in one call ->
profiles/r27/noise.json.  Set and protocol are those of tools/light_bench.py (its frames, its model, device events, windows
alternating in one call).
  (a) kernel: 1024 resident 1280x1024 synth frames in 25 stacks with a model, every frame against the frame two before it in
      its stack (the first two of a stack against frame 0 of it) on the grid of R = 4 (9 x 7 cells); three launches per
      window, five windows alternating with abub_frame_light_cells_dev on the same frames; ms per launch (median and range),
      the ratio of the two, frames per second, and the bytes moved per second: p and r are frame bytes that every job reads
      for itself (2 * cells * 16384 per frame, from HBM unless the pair's other job left them in a cache), sigma6 is one
      plane that every frame reads again, most likely from a cache, so the rate is given with and without it; the fraction
      of a read ceiling is left to the reader of the JSON, who has the ceiling's figure; some records are checked against
      noiseCellsHost first;
  (c) end to end: the 1025-frame run of survey_bench part (c), as PNG files and repacked, surveyed by the CLI on the host
      route and with --survey-gpu, with --survey-noise and without, each three times alternating, from the page cache;
      medians of the CLI's own seconds; the noise's files and the reports compared byte for byte; the kinds noise.txt gives
      this steady run and the baseline's bias (the rated cells' q_milli of the rows that are not the baseline's own);
  (d) parent comparison: bench.py --steps 20 --warmup 5, parent build and this tree in the balanced twelve-run order of
      tools/verify_bench.py, dumped outputs compared byte for byte.
usage: python3 tools/noise_bench.py [--parts acd] [--parent PARENT_CHECKOUT] [--balanced [ORDER]] [--out profiles/r27/noise.json]
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
    ref = [i - 2 if fr[i][1] >= 2 else i - fr[i][1] for i in range(n)]
    pairs = np.array([[i * P, ref[i] * P, 0] for i in range(n)], dtype=np.int64)
    jobs = np.array([[i * P, 0] for i in range(n)], dtype=np.int64)
    ncx, ncy, x0, y0 = hip.field_grid(W, H, R)
    cells = ncx * ncy
    status, rec = hip.frame_noise_cells(slab, d_s6, pairs, W, H, x0, y0, ncx, ncy)
    assert not status.any()
    for i in (0, 1, F - 1, n - 1):
        assert np.array_equal(rec[i], host.noise_cells_host(fr[i][2], fr[ref[i]][2], s6, x0, y0, ncx, ncy)), i
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    d_jobs, d_pairs = torch.from_numpy(jobs).to(dev), torch.from_numpy(pairs).to(dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    out = torch.empty((n * cells * 6,), dtype=torch.int32, device=dev)

    def noise(rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_noise_cells_dev(slab.data_ptr(), slab.numel(), d_s6.data_ptr(), d_s6.numel(), d_pairs.data_ptr(), n, W,
                                                    H, x0, y0, ncx, ncy, status.data_ptr(), out.data_ptr(), stream), "noise")

    def light(rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_light_cells_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_mu.numel(), d_jobs.data_ptr(), n, W,
                                                    H, x0, y0, ncx, ncy, status.data_ptr(), out.data_ptr(), stream), "light")

    def timed(fn, rep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(rep)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / rep

    kernels = {"noise": noise, "light": light}
    for fn in kernels.values():
        fn(1)
    torch.cuda.synchronize()
    t = {k: [] for k in kernels}
    for _ in range(5):
        for k, fn in kernels.items():
            t[k].append(timed(fn, 3))
    med = {k: statistics.median(v) for k, v in t.items()}
    in_cells = cells * 16384
    rate = lambda streams, ms: streams * in_cells * n / ms * 1e3 / 1e9  # noqa: E731
    return {"frames": n, "W": W, "H": H, "grid": [ncx, ncy, x0, y0], "cells": cells, "launches_per_window": 3, "windows": 5,
            "ms_per_launch": t, "ms_per_launch_median": med, "ms_per_launch_range": {k: [min(v), max(v)] for k, v in t.items()},
            "frames_per_s": n / med["noise"] * 1e3, "noise_over_light_time": med["noise"] / med["light"],
            "bytes_in_the_cells_per_frame_and_stream": in_cells,
            "noise_GB_per_s": {"p_and_r": rate(2, med["noise"]), "p_r_and_sigma6": rate(3, med["noise"])},
            "light_GB_per_s": {"p": rate(1, med["light"]), "p_and_mu": rate(2, med["light"])},
            "rate_note": "p and r are frame bytes (r is the p of another job of the same launch); sigma6 and mu are one plane read again "
                         "by every frame, most likely from a cache: only the frame bytes can be set against an HBM read ceiling"}


def noise_txt_summary(text):
    """the kinds of the rows that have a record, and the q_milli of the rated cells: of the baseline's own rows (stack
    position 1) and of the others"""
    rows = [l.split("\t") for l in text.splitlines()[3:] if "\t" in l]
    made = [r for r in rows if r[5] != "-"]
    kinds = {}
    for r in made:
        kinds[r[15]] = kinds.get(r[15], 0) + 1
    q = lambda sel: sorted(int(r[11]) for r in made if r[11] != "-" and sel(r))  # noqa: E731
    own, others = q(lambda r: r[2] == "1"), q(lambda r: r[2] != "1")
    rng = lambda v: {"n": len(v), "min": v[0], "median": v[len(v) // 2], "max": v[-1]} if v else {"n": 0}  # noqa: E731
    return {"rows_with_a_record": len(made), "kinds": kinds, "changed_cells": sum(int(r[9]) + int(r[10]) for r in made),
            "busy_cells": sum(int(r[8]) for r in made), "pooled_q_milli_of_the_baseline_rows": rng(own), "pooled_q_milli_of_the_other_rows": rng(others),
            "cam_line": [l for l in text.splitlines() if l.startswith("noise cam")]}


def part_c(n):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image

    run_id = "20200925_0"
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="1", ABUB_THREADS="16")
    tmp = tempfile.mkdtemp(prefix="abub_noise_")
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
        out, reports, noises, text = {}, set(), set(), None
        configs = [(route, flag) for flag in (True, False) for route in ("host", "gpu")]
        for kind in ("png", "packed"):
            series = {f"{route}{'_noise' if fl else ''}": [] for route, fl in configs}
            lines = {}
            for rep in range(3):
                for route, fl in configs:
                    key = f"{route}{'_noise' if fl else ''}"
                    rep_file, noise_dir = os.path.join(tmp, f"{kind}_{key}.txt"), os.path.join(tmp, f"{kind}_{key}_noise")
                    args = [exe, "-d", os.path.join(tmp, kind), "-r", run_id, "--survey", rep_file]
                    args += ["--survey-noise", noise_dir] if fl else []
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
                        d = os.path.join(noise_dir, run_id)
                        noises.add(tuple(open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))))
                        text = open(os.path.join(d, "noise.txt")).read()
            med = {k: statistics.median(x["survey_s"] for x in v) for k, v in series.items()}
            out[kind] = {"runs": series, "survey_s_median": med, "survey_s_range": {k: [min(x["survey_s"] for x in v), max(x["survey_s"] for x in v)]
                                                                                    for k, v in series.items()},
                         "frames_per_s": {k: n / v for k, v in med.items()},
                         "gpu_over_host_with_noise": med["host_noise"] / med["gpu_noise"], "gpu_over_host_without": med["host"] / med["gpu"],
                         "noise_adds_s": {"host": med["host_noise"] - med["host"], "gpu": med["gpu_noise"] - med["gpu"]}, "last_lines": lines}
        out["reports_identical"] = len(reports) == 1
        out["noise_files_identical"] = len(noises) == 1
        out["frames"] = n
        out["noise_txt_of_this_steady_run"] = noise_txt_summary(text)
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="acd")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27", "noise.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--balanced", nargs="?", const="TPPTTPPTTPPT", default="TPPTTPPTTPPT")
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):  # (a call that measures some of the parts keeps the others)
        result = json.load(open(a.out))
    for part, fn in (("a", lambda: part_a(a.frames)), ("c", lambda: part_c(a.frames)), ("d", lambda: part_d(a.parent, a.balanced))):
        key = {"a": "kernel", "c": "end_to_end", "d": "parent_comparison_" + a.balanced}[part]
        if part not in a.parts or (part == "d" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
