#!/usr/bin/env python3
"""abub_frame_shift_cells_dev and abub3hs --survey --survey-field [--survey-gpu] measured on one GPU box, in one call ->
profiles/r23/field.json.  Set and protocol are those of tools/survey_bench.py and tools/shift_bench.py (their frames, their
model, device events, windows alternating in one call).
  (a) kernel: 1024 resident 1280x1024 synth frames in 25 stacks with a model, every frame against mu at R = 2, 4 and 8; three
      launches per window, five windows alternating with abub_frame_shift_dev at the same radius on the same frames; ms per
      launch (median and range), frames per second, packed-SAD operations per second against the count (2R+1)^2 * cells *
      16384 / 4 per frame, and the ratio to the frame kernel; some surfaces are checked against fieldCellsHost first;
  (c) end to end: the 1025-frame run of survey_bench part (c), as PNG files and repacked, surveyed by the CLI on the host
      route and with --survey-gpu, with --survey-field and without, each three times alternating, from the page cache;
      medians of the CLI's own seconds; the field's files and the reports compared byte for byte;
  (d) parent comparison: bench.py --steps 20 --warmup 5, parent build and this tree in the balanced twelve-run order of
      tools/verify_bench.py, dumped outputs compared byte for byte;
  (e) the committed sample frame of the 40l-19 data (tests/golden) as a three-frame event whose third frame is rotated by
      0.1 degrees on the host (Pillow, bicubic): field.txt and the shift file's rows of both routes.
usage: python3 tools/field_bench.py [--parts acde] [--parent PARENT_CHECKOUT] [--balanced [ORDER]] [--out profiles/r23/field.json]
                                    [--frames 1024]"""
import argparse, io, json, os, shutil, statistics, subprocess, sys, tempfile, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from survey_bench import F, H, P, W, model_of, part_d, stacks  # noqa: E402

RADII = (2, 4, 8)


def part_a(n):
    import torch
    from autobub3hs_amd import _lib, hip, host

    fr = stacks(n)
    mu, _, _ = model_of(fr)
    dev = torch.device("cuda:0")
    slab = torch.empty((n, P), dtype=torch.uint8, device=dev)
    for i, (_, _, f) in enumerate(fr):
        slab[i] = torch.from_numpy(f.reshape(-1)).to(dev)
    slab = slab.reshape(-1)
    d_mu = torch.from_numpy(mu.reshape(-1)).to(dev)
    jobs = np.array([[i * P, 0] for i in range(n)], dtype=np.int64)
    cells = {}
    for R in RADII:
        ncx, ncy, _, _ = hip.field_grid(W, H, R)
        cells[R] = ncx * ncy
        status, sad = hip.frame_shift_cells(slab, d_mu, jobs, W, H, R)
        assert not status.any()
        for i in (0, F - 1, n - 1):
            assert np.array_equal(sad[i], host.field_cells_host(fr[i][2], mu, R)[0]), (R, i)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    d_jobs = torch.from_numpy(jobs).to(dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    surf = torch.empty((n * 17 * 17,), dtype=torch.int64, device=dev)
    csurf = torch.empty((n * max(cells.values()) * 17 * 17,), dtype=torch.int32, device=dev)

    def frame(R, rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_shift_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_mu.numel(), d_jobs.data_ptr(), n, W, H, R,
                                              status.data_ptr(), surf.data_ptr(), stream), "shift")

    def field(R, rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_shift_cells_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_mu.numel(), d_jobs.data_ptr(), n, W,
                                                    H, R, status.data_ptr(), csurf.data_ptr(), stream), "cells")

    def timed(fn, rep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(rep)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / rep

    for R in RADII:
        frame(R, 1)
        field(R, 1)
    torch.cuda.synchronize()
    t = {f"{k}_R{R}": [] for R in RADII for k in ("cells", "frame")}
    for _ in range(5):
        for R in RADII:
            t[f"cells_R{R}"].append(timed(lambda rep, R=R: field(R, rep), 3))
            t[f"frame_R{R}"].append(timed(lambda rep, R=R: frame(R, rep), 3))
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"frames": n, "W": W, "H": H, "launches_per_window": 3, "windows": 5, "ms_per_launch": t, "ms_per_launch_median": med,
           "ms_per_launch_range": {k: [min(v), max(v)] for k, v in t.items()}}
    for R in RADII:
        ops = (2 * R + 1) ** 2 * cells[R] * 16384 / 4.0
        ms = med[f"cells_R{R}"]
        out[f"R{R}"] = {"cells": cells[R], "pixels_summed_share": cells[R] * 16384 / float((W - 2 * R) * (H - 2 * R)),
                        "frames_per_s": n / ms * 1e3, "packed_sad_ops_per_frame": ops, "packed_sad_ops_per_s": ops * n / ms * 1e3,
                        "cells_over_frame_time": ms / med[f"frame_R{R}"]}
    return out


def part_c(n):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image

    run_id = "20200925_0"
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="1", ABUB_THREADS="16")
    tmp = tempfile.mkdtemp(prefix="abub_field_")
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
        out, reports, fields = {}, set(), set()
        configs = [(route, with_field) for with_field in (True, False) for route in ("host", "gpu")]
        for kind in ("png", "packed"):
            series = {f"{route}{'_field' if fl else ''}": [] for route, fl in configs}
            lines = {}
            for rep in range(3):
                for route, fl in configs:
                    key = f"{route}{'_field' if fl else ''}"
                    rep_file, field_dir = os.path.join(tmp, f"{kind}_{key}.txt"), os.path.join(tmp, f"{kind}_{key}_field")
                    args = [exe, "-d", os.path.join(tmp, kind), "-r", run_id, "--survey", rep_file]
                    args += ["--survey-field", field_dir] if fl else []
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
                        d = os.path.join(field_dir, run_id)
                        fields.add(tuple(open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))))
            med = {k: statistics.median(x["survey_s"] for x in v) for k, v in series.items()}
            out[kind] = {"runs": series, "survey_s_median": med, "frames_per_s": {k: n / v for k, v in med.items()},
                         "gpu_over_host_with_field": med["host_field"] / med["gpu_field"], "gpu_over_host_without": med["host"] / med["gpu"],
                         "field_adds_s": {"host": med["host_field"] - med["host"], "gpu": med["gpu_field"] - med["gpu"]}, "last_lines": lines}
        out["reports_identical"] = len(reports) == 1
        out["field_files_identical"] = len(fields) == 1
        out["frames"] = n
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def part_e():
    from PIL import Image

    run_id = "20200925_0"
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    image = Image.open(os.path.join(ROOT, "tests", "golden", "sample_40l19_cam1_image30.png")).convert("L")
    sample = np.array(image)
    h, w = sample.shape
    angle = 0.1
    turned = np.array(image.rotate(angle, resample=Image.BICUBIC))
    tmp = tempfile.mkdtemp(prefix="abub_field_sample_")
    try:
        d = os.path.join(tmp, run_id, "0", "Images")
        os.makedirs(d)
        for k, img in enumerate((sample, sample, turned)):
            Image.fromarray(img).save(os.path.join(d, f"cam1_image{30 + k}.png"))
        texts, shifts = [], []
        for flag in ([], ["--survey-gpu"]):
            rep, sh, fd = os.path.join(tmp, "report.txt"), os.path.join(tmp, "shift.txt"), os.path.join(tmp, "field")
            r = subprocess.run([exe, "-d", tmp, "-r", run_id, "-D", "40l-19", "--survey", rep, "--survey-shift", sh, "--survey-field", fd] + flag,
                               env=dict(os.environ, ABUB_NUM_CAMS="2"), capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            texts.append(open(os.path.join(fd, run_id, "field.txt")).read())
            shifts.append(open(sh).read())
            rec = np.load(os.path.join(fd, run_id, "cam1_field.npy"))
        assert texts[0] == texts[1] and shifts[0] == shifts[1]
        return {"frames": 3, "W": int(w), "H": int(h), "rotated_degrees": angle, "resample": "bicubic", "routes_identical": True,
                "field_txt": texts[0].splitlines(), "shift_file": shifts[0].splitlines(),
                "third_frame_dx": rec[2, :, :, 0].tolist(), "third_frame_dy": rec[2, :, :, 1].tolist(),
                "third_frame_rated": [[bool(c[4] > 0 and 2 * int(c[3]) <= int(c[4])) for c in row] for row in rec[2]]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="acde")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "field.json"))
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
