#!/usr/bin/env python3
"""abub_frame_shift_dev and abub3hs --survey --survey-shift [--survey-gpu] measured on one GPU box, in one call ->
profiles/r22/shift.json.  Set and protocol are those of tools/survey_bench.py (its frames, its model, device events, windows
alternating in one call).
  (a) kernel: 1024 resident 1280x1024 synth frames in 25 stacks with a model, every frame against mu at R = 4, 2 and 8; three
      launches per window, five windows alternating with abub_frame_stats_dev on the same frames (ten launches per window);
      ms per launch, frames per second, and packed-SAD operations per second against the count (2R+1)^2 |I| / 4 per frame
      (what the arithmetic needs, not what the kernel issues: a lane at the interior's right edge, and the masked path's
      v_and_b32, are not in it); some surfaces are checked against frameShiftHost first;
  (b) frameShiftHost on 16 threads over the first 256 of those frames, at R = 4;
  (c) end to end: the 1025-frame run of survey_bench part (c), as PNG files and repacked, surveyed by the CLI on the host
      route and with --survey-gpu, with --survey-shift and without, each three times alternating, from the page cache;
      medians of the CLI's own seconds; the shift files and the reports compared byte for byte;
  (d) parent comparison: bench.py --steps 20 --warmup 5, parent build and this tree in the balanced twelve-run order of
      tools/verify_bench.py, dumped outputs compared byte for byte;
  (e) the committed sample frame of the 40l-19 data (tests/golden) as a three-frame event whose third frame is displaced by
      (3, -2) on the host (edge pixels repeated): the shift rows of both routes.
usage: python3 tools/shift_bench.py [--parts abcde] [--parent PARENT_CHECKOUT] [--balanced [ORDER]] [--out profiles/r22/shift.json]
                                    [--frames 1024]"""
import argparse, io, json, os, shutil, statistics, subprocess, sys, tempfile, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from survey_bench import F, H, P, W, model_of, part_d, stacks  # noqa: E402

RADII = (4, 2, 8)


def part_a(n):
    import torch
    from autobub3hs_amd import _lib, hip, host

    fr = stacks(n)
    mu, sg, s6 = model_of(fr)
    dev = torch.device("cuda:0")
    slab = torch.empty((n, P), dtype=torch.uint8, device=dev)
    for i, (_, _, f) in enumerate(fr):
        slab[i] = torch.from_numpy(f.reshape(-1)).to(dev)
    slab = slab.reshape(-1)
    d_mu, d_s6 = torch.from_numpy(mu.reshape(-1)).to(dev), torch.from_numpy(s6.reshape(-1)).to(dev)
    jobs = np.array([[i * P, 0] for i in range(n)], dtype=np.int64)
    for R in RADII:
        status, sad = hip.frame_shift(slab, d_mu, jobs, W, H, R)
        assert not status.any()
        for i in (0, F - 1, n - 1):
            assert np.array_equal(sad[i], host.frame_shift_host(fr[i][2], mu, R)), (R, i)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    d_jobs = torch.from_numpy(jobs).to(dev)
    stat_jobs = torch.from_numpy(np.array([[i * P, (i - min(k, 2)) * P, 0] for i, (_, k, _) in enumerate(fr)], dtype=np.int64)).to(dev)
    res = torch.empty((n * 64,), dtype=torch.uint8, device=dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    surf = torch.empty((n * 17 * 17,), dtype=torch.int64, device=dev)

    def shift(R, rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_shift_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_mu.numel(), d_jobs.data_ptr(), n, W, H, R,
                                              status.data_ptr(), surf.data_ptr(), stream), "shift")

    def stats(rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_stats_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_s6.data_ptr(), P, stat_jobs.data_ptr(), n, P,
                                              res.data_ptr(), stream), "stats")

    def timed(fn, rep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(rep)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / rep

    for R in RADII:
        shift(R, 1)
    stats(1)
    torch.cuda.synchronize()
    t = {f"shift_R{R}": [] for R in RADII}
    t["stats"] = []
    for _ in range(5):
        for R in RADII:
            t[f"shift_R{R}"].append(timed(lambda rep, R=R: shift(R, rep), 3))
            t["stats"].append(timed(stats, 10))
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"frames": n, "W": W, "H": H, "ms_per_launch": t, "ms_per_launch_median": med, "launches_per_window": {"shift": 3, "stats": 10}}
    for R in RADII:
        ops = (2 * R + 1) ** 2 * (W - 2 * R) * (H - 2 * R) / 4.0
        ms = med[f"shift_R{R}"]
        out[f"R{R}"] = {"frames_per_s": n / ms * 1e3, "ms_per_frame": ms / n, "packed_sad_ops_per_frame": ops,
                        "packed_sad_ops_per_s": ops * n / ms * 1e3, "over_stats_time": ms / med["stats"]}
    return out


def part_b(n, threads=16, R=4):
    from concurrent.futures import ThreadPoolExecutor
    from autobub3hs_amd import host

    n = min(n, 256)
    fr = stacks(n)
    mu, _, _ = model_of(fr)
    one = lambda i: host.frame_shift_host(fr[i][2], mu, R)  # noqa: E731
    times = []
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(min(32, n))))
        for _ in range(3):
            t0 = time.perf_counter()
            list(ex.map(one, range(n)))
            times.append(time.perf_counter() - t0)
    s = statistics.median(times)
    return {"frames": n, "threads": threads, "R": R, "seconds": times, "frames_per_s": n / s, "thread_ms_per_frame": s * threads / n * 1e3}


def part_c(n):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image

    run_id = "20200925_0"
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="1", ABUB_THREADS="16")
    tmp = tempfile.mkdtemp(prefix="abub_shift_")
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
        out, reports, shifts = {}, set(), set()
        configs = [(route, with_shift) for with_shift in (True, False) for route in ("host", "gpu")]
        for kind in ("png", "packed"):
            series = {f"{route}{'_shift' if sh else ''}": [] for route, sh in configs}
            lines = {}
            for rep in range(3):
                for route, sh in configs:
                    key = f"{route}{'_shift' if sh else ''}"
                    rep_file, shift_file = os.path.join(tmp, f"{kind}_{key}.txt"), os.path.join(tmp, f"{kind}_{key}.shift.txt")
                    args = [exe, "-d", os.path.join(tmp, kind), "-r", run_id, "--survey", rep_file]
                    args += ["--survey-shift", shift_file] if sh else []
                    args += ["--survey-gpu"] if route == "gpu" else []
                    t0 = time.perf_counter()
                    r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=1200)
                    wall = time.perf_counter() - t0
                    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
                    line = [l for l in r.stdout.splitlines() if l.startswith("survey: ")][-1]
                    series[key].append({"survey_s": float(line.rsplit("; ", 1)[1].split(" s,")[0]), "process_s": wall})
                    lines[key] = [l.replace(tmp, "TMP") for l in r.stdout.splitlines() if l.startswith("survey")]
                    reports.add(open(rep_file, "rb").read())
                    if sh:
                        shifts.add(open(shift_file, "rb").read())
            med = {k: statistics.median(x["survey_s"] for x in v) for k, v in series.items()}
            out[kind] = {"runs": series, "survey_s_median": med, "frames_per_s": {k: n / v for k, v in med.items()},
                         "gpu_over_host_with_shift": med["host_shift"] / med["gpu_shift"], "gpu_over_host_without": med["host"] / med["gpu"],
                         "shift_adds_s": {"host": med["host_shift"] - med["host"], "gpu": med["gpu_shift"] - med["gpu"]}, "last_lines": lines}
        out["reports_identical"] = len(reports) == 1
        out["shift_files_identical"] = len(shifts) == 1
        text = shifts.pop().decode().splitlines()
        out["shift_file_tail"] = text[-2:]
        out["frames"] = n
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def part_e():
    from PIL import Image

    run_id = "20200925_0"
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    sample = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "sample_40l19_cam1_image30.png")).convert("L"))
    dx, dy, m = 3, -2, 4
    big = np.pad(sample, m, mode="edge")
    h, w = sample.shape
    moved = np.ascontiguousarray(big[m - dy:m - dy + h, m - dx:m - dx + w])  # moved(x + dx, y + dy) == sample(x, y)
    tmp = tempfile.mkdtemp(prefix="abub_shift_sample_")
    try:
        d = os.path.join(tmp, run_id, "0", "Images")
        os.makedirs(d)
        for k, img in enumerate((sample, sample, moved)):
            Image.fromarray(img).save(os.path.join(d, f"cam1_image{30 + k}.png"))
        texts = []
        for flag in ([], ["--survey-gpu"]):
            rep, sh = os.path.join(tmp, "report.txt"), os.path.join(tmp, "shift.txt")
            r = subprocess.run([exe, "-d", tmp, "-r", run_id, "-D", "40l-19", "--survey", rep, "--survey-shift", sh] + flag,
                               env=dict(os.environ, ABUB_NUM_CAMS="2"), capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            texts.append(open(sh).read())
        assert texts[0] == texts[1]
        return {"frames": 3, "W": int(w), "H": int(h), "displaced": [dx, dy], "routes_identical": True, "shift_file": texts[0].splitlines()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abcde")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "shift.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--balanced", nargs="?", const="TPPTTPPTTPPT", default="TPPTTPPTTPPT")
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):  # (a call that measures some of the parts keeps the others)
        result = json.load(open(a.out))
    for part, fn in (("a", lambda: part_a(a.frames)), ("b", lambda: part_b(a.frames)), ("c", lambda: part_c(a.frames)),
                     ("e", part_e), ("d", lambda: part_d(a.parent, a.balanced))):
        key = {"a": "kernel", "b": "host_definition", "c": "end_to_end", "d": "parent_comparison_" + a.balanced, "e": "sample_frame_run"}[part]
        if part not in a.parts or (part == "d" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
