#!/usr/bin/env python3
"""abub_pixel_activity_dev and abub3hs --survey --survey-planes measured on one GPU box, in one call -> profiles/r21/activity.json.
  (a) kernel: tools/survey_bench.py's set (1024 resident 1280 x 1024 synth frames in 25 stacks of 41 with a model, every frame
      against the frame two before it); abub_pixel_activity_dev alternates with abub_frame_stats_dev on the same frames: ten
      launches per window, five windows, device events, medians; ms, frames/s, TB/s on compulsory bytes (each frame once, the
      model once, the planes read and written once) and on requested bytes as launched (two streams per job, the model once,
      the planes); the result is checked against the stats kernel's records first (plane totals = column sums);
  (c) end to end: survey_bench's run (1025 frames as 25 events of one camera, PNG files and the packed copy), --survey against
      --survey --survey-planes, with --survey-gpu on both copies and on the host route on the packed copy, three alternating
      repetitions, medians; the added time and its legs (activity launches, copy back, files) from the CLI's own line; the
      files of the two routes compared byte for byte.
usage: python3 tools/activity_bench.py [--parts ac] [--out profiles/r21/activity.json] [--frames 1024]"""
import argparse, io, json, os, shutil, statistics, subprocess, sys, tempfile, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from survey_bench import F, H, P, W, model_of, stacks  # noqa: E402


def part_a(n):
    import torch
    from autobub3hs_amd import _lib, hip

    fr = stacks(n)
    mu, sg, s6 = model_of(fr)
    dev = torch.device("cuda:0")
    slab = torch.empty((n, P), dtype=torch.uint8, device=dev)
    for i, (_, _, f) in enumerate(fr):
        slab[i] = torch.from_numpy(f.reshape(-1)).to(dev)
    slab = slab.reshape(-1)
    d_mu, d_s6 = torch.from_numpy(mu.reshape(-1)).to(dev), torch.from_numpy(s6.reshape(-1)).to(dev)
    jobs = np.array([[i * P, (i - min(k, 2)) * P, 0] for i, (_, k, _) in enumerate(fr)], dtype=np.int64)
    planes = torch.zeros((6, P), dtype=torch.int32, device=dev)
    assert hip.pixel_activity(slab, jobs[:, :2], P, planes, d_mu, d_s6) == 0
    rec = hip.frame_stats(slab, jobs, P, d_mu, d_s6)
    cols = {name: k for k, name in enumerate(hip.STAT_COLUMNS)}
    totals = planes.cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=1)
    assert [int(v) for v in totals] == [int(rec[:, cols[name]].sum()) for name in hip.ACT_PLANES], "plane totals != column sums"
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    d_jobs = torch.from_numpy(jobs).to(dev)
    d_act = torch.from_numpy(np.ascontiguousarray(jobs[:, :2])).to(dev)
    res = torch.empty((n * 64,), dtype=torch.uint8, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    REP = 10

    def stats():
        for _ in range(REP):
            _lib.check(L.abub_frame_stats_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_s6.data_ptr(), P, d_jobs.data_ptr(), n, P,
                                              res.data_ptr(), stream), "stats")

    def activity():
        for _ in range(REP):
            _lib.check(L.abub_pixel_activity_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_s6.data_ptr(), d_act.data_ptr(), n, P,
                                                 planes.data_ptr(), P, status.data_ptr(), stream), "activity")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REP

    for fn in (stats, activity):
        fn()
    torch.cuda.synchronize()
    t = {"activity": [], "stats": []}
    for _ in range(5):
        t["activity"].append(timed(activity))
        t["stats"].append(timed(stats))
    med = {k: statistics.median(v) for k, v in t.items()}
    compulsory = n * P + 2 * P + 2 * 24 * P
    requested = 2 * n * P + 2 * P + 2 * 24 * P
    return {"frames": n, "W": W, "H": H, "stacks": (n + F - 1) // F, "launches_per_window": REP, "ms_per_launch": t,
            "ms_per_launch_median": med, "frames_per_s": n / med["activity"] * 1e3, "compulsory_bytes": compulsory,
            "TBps_on_compulsory_bytes": compulsory / med["activity"] / 1e9, "requested_bytes": requested,
            "TBps_on_requested_bytes": requested / med["activity"] / 1e9, "stats_frames_per_s": n / med["stats"] * 1e3,
            "activity_over_stats_time": med["activity"] / med["stats"], "plane_totals_equal_column_sums": True}


def part_c(n):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image

    run_id = "20200925_0"
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="1", ABUB_THREADS="16")
    tmp = tempfile.mkdtemp(prefix="abub_activity_")
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
        out, files, reports = {}, set(), set()
        for kind, route, flag in (("packed", "gpu", ["--survey-gpu"]), ("png", "gpu", ["--survey-gpu"]), ("packed", "host", [])):
            series = {"bare": [], "planes": []}
            last = None
            for rep in range(3):
                for what in ("bare", "planes"):
                    rep_file = os.path.join(tmp, f"{kind}_{route}_{what}.txt")
                    pdir = os.path.join(tmp, f"planes_{kind}_{route}")
                    more = ["--survey-planes", pdir] if what == "planes" else []
                    t0 = time.perf_counter()
                    r = subprocess.run([exe, "-d", os.path.join(tmp, kind), "-r", run_id, "--survey", rep_file] + flag + more, env=env,
                                       capture_output=True, text=True, timeout=900)
                    wall = time.perf_counter() - t0
                    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
                    line = [l for l in r.stdout.splitlines() if l.startswith("survey: ")][-1]
                    series[what].append({"survey_s": float(line.rsplit("; ", 1)[1].split(" s,")[0]), "process_s": wall})
                    reports.add(open(rep_file, "rb").read())
                    if what == "planes":
                        last = [l for l in r.stdout.splitlines() if l.startswith("survey-planes: ")][-1].split(": ", 2)[2]
                        d = os.path.join(pdir, run_id)
                        files.add(tuple((f, open(os.path.join(d, f), "rb").read()) for f in sorted(os.listdir(d)) if not f.endswith(".png")))
                        activity_txt = open(os.path.join(d, "activity.txt")).read().splitlines()
            med = {k: statistics.median(x["survey_s"] for x in v) for k, v in series.items()}
            out[f"{kind}_{route}"] = {"runs": series, "survey_s_median": med, "added_s": med["planes"] - med["bare"],
                                      "planes_over_bare": med["planes"] / med["bare"], "legs": last}
        out["reports_identical"] = len(reports) == 1
        out["npy_and_txt_identical_on_all_routes"] = len(files) == 1
        out["activity_txt_head"] = activity_txt[:6]
        out["frames"] = n
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ac")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "activity.json"))
    ap.add_argument("--frames", type=int, default=1024)
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):  # (a call that measures some of the parts keeps the others)
        result = json.load(open(a.out))
    for part, key, fn in (("a", "kernel", lambda: part_a(a.frames)), ("c", "end_to_end", lambda: part_c(a.frames))):
        if part not in a.parts:
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
