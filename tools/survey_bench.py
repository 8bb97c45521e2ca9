#!/usr/bin/env python3
"""abub_frame_stats_dev and abub3hs --survey [--survey-gpu] measured on one GPU box, in one call -> profiles/r20/survey.json.
  (a) kernel: 1024 resident 1280x1024 synth frames in 25 stacks of 41 (the last of 40) with a model, every frame against the
      frame two before it in its stack; ten launches per window, five windows alternating with abub_frames_compare_dev on the
      same frame count (identical frames: its fast path, the yardstick for a read of two streams), device events, medians;
      frames per second and TB/s on the compulsory bytes (each frame once, the model's two planes once per camera); the
      same without a model (one stream); the records are checked against frameStatsHost first;
  (b) frameStatsHost on 16 threads over the same frames (the model and the reference frame given);
  (c) end to end: that run with its last stack filled up (1025 frames) as 25 events of one camera, as PNG files and repacked (--repack), surveyed by the CLI on the host
      route and with --survey-gpu, each three times alternating, from the page cache; the reports compared byte for byte;
  (d) parent comparison: tools/abf_bench.py part (c) (bench.py --steps 20 --warmup 5, parent build and this tree alternating,
      three runs each, dumped outputs compared byte for byte); --balanced [ORDER]: twelve runs in the balanced order
      T P P T ... of tools/verify_bench.py instead (or in ORDER);
  (e) the report of the committed sample frame of the 40l-19 data (tests/golden) as a one-event run of three copies of it.
usage: python3 tools/survey_bench.py [--parts abcde] [--parent PARENT_CHECKOUT] [--balanced [ORDER]] [--out profiles/r20/survey.json] [--frames 1024]"""
import argparse, io, json, os, shutil, statistics, subprocess, sys, tempfile, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

W, H, F = 1280, 1024, 41
P = W * H


def stacks(n):
    """the frames of the run: stack s, frame k -> the synth frame k of event s (25 distinct events would take minutes to
    render: five are rendered and reused, which changes no byte count)"""
    from autobub3hs_amd import synth

    ev = [np.asarray(synth.render_event(W, H, synth.random_spec(W, H, F, e, 0, p_second=0.2), e, 0)) for e in range(5)]
    return [(i // F, i % F, ev[(i // F) % 5][i % F]) for i in range(n)]


def model_of(frames):
    """a model as the Trainer makes it, by the oracle's Welford pass over the first two frames of every stack"""
    from oracle import pyoracle as orc

    tr = np.stack([f for s, k, f in frames if k < 2])
    mu, sg = orc.welford(tr)
    return mu, sg, np.minimum(sg.astype(np.int64) * 6, 255).astype(np.uint8)


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
    jobs = np.array([[i * P, (i - min(k, 2)) * P, 0] for i, (_, k, _) in enumerate(fr)], dtype=np.int64)
    got = hip.frame_stats(slab, jobs, P, d_mu, d_s6)
    for i in (0, 1, 2, F - 1, F, n - 1):
        want = host.frame_stats_host(fr[i][2], fr[i - min(fr[i][1], 2)][2], mu, s6)
        assert got[i, 0] == 0 and [int(v) for v in got[i, 1:]] == [want[k] for k in host.FRAME_STATS_KEYS], i
    bare = jobs.copy()
    bare[:, 1:] = -1
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    d_jobs = torch.from_numpy(jobs).to(dev)
    d_bare = torch.from_numpy(bare).to(dev)
    res = torch.empty((n * 64,), dtype=torch.uint8, device=dev)
    pairs = torch.from_numpy(np.stack([jobs[:, 0], jobs[:, 0]], axis=1)).to(dev)  # the same frames on both sides
    other = slab.clone()
    cres = torch.empty((n, 4), dtype=torch.int32, device=dev)
    REP = 10

    def stats(j, with_model):
        for _ in range(REP):
            _lib.check(L.abub_frame_stats_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr() if with_model else None, d_s6.data_ptr(),
                                              P, j.data_ptr(), n, P, res.data_ptr(), stream), "stats")

    def compare():
        for _ in range(REP):
            _lib.check(L.abub_frames_compare_dev(slab.data_ptr(), slab.numel(), other.data_ptr(), other.numel(), pairs.data_ptr(), n, P,
                                                 cres.data_ptr(), stream), "cmp")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REP

    for fn in (lambda: stats(d_jobs, True), lambda: stats(d_bare, False), compare):
        fn()
    torch.cuda.synchronize()
    t = {"model_and_reference": [], "frame_alone": [], "compare": []}
    for _ in range(5):
        t["model_and_reference"].append(timed(lambda: stats(d_jobs, True)))
        t["compare"].append(timed(compare))
        t["frame_alone"].append(timed(lambda: stats(d_bare, False)))
    med = {k: statistics.median(v) for k, v in t.items()}
    compulsory = n * P + 2 * P
    return {"frames": n, "W": W, "H": H, "stacks": (n + F - 1) // F, "launches_per_window": REP, "ms_per_launch": t,
            "ms_per_launch_median": med, "frames_per_s": n / med["model_and_reference"] * 1e3,
            "compulsory_bytes": compulsory, "TBps_on_compulsory_bytes": compulsory / med["model_and_reference"] / 1e9,
            "frame_alone_frames_per_s": n / med["frame_alone"] * 1e3, "frame_alone_TBps": n * P / med["frame_alone"] / 1e9,
            "compare_bytes": 2 * n * P, "compare_TBps": 2 * n * P / med["compare"] / 1e9,
            "compare_pairs_per_s": n / med["compare"] * 1e3, "stats_over_compare_time": med["model_and_reference"] / med["compare"]}


def part_b(n, threads=16):
    from concurrent.futures import ThreadPoolExecutor
    from autobub3hs_amd import host

    fr = stacks(n)
    mu, sg, s6 = model_of(fr)
    one = lambda i: host.frame_stats_host(fr[i][2], fr[i - min(fr[i][1], 2)][2], mu, s6)  # noqa: E731
    times = []
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(one, range(min(64, n))))
        for _ in range(3):
            t0 = time.perf_counter()
            list(ex.map(one, range(n)))
            times.append(time.perf_counter() - t0)
    s = statistics.median(times)
    return {"frames": n, "threads": threads, "seconds": times, "frames_per_s": n / s}


def part_c(n):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image

    run_id = "20200925_0"
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="1", ABUB_THREADS="16")
    tmp = tempfile.mkdtemp(prefix="abub_survey_")
    try:
        n = (n + F - 1) // F * F  # (whole stacks: a stack that ends early would be a run with missing frames)
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
        out, reports = {}, set()
        for kind in ("png", "packed"):
            series = {"host": [], "gpu": []}
            lines = {}
            for rep in range(3):
                for route, flag in (("host", []), ("gpu", ["--survey-gpu"])):
                    rep_file = os.path.join(tmp, f"{kind}_{route}.txt")
                    t0 = time.perf_counter()
                    r = subprocess.run([exe, "-d", os.path.join(tmp, kind), "-r", run_id, "--survey", rep_file] + flag, env=env,
                                       capture_output=True, text=True, timeout=900)
                    wall = time.perf_counter() - t0
                    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
                    line = [l for l in r.stdout.splitlines() if l.startswith("survey: ")][-1]
                    secs = float(line.rsplit("; ", 1)[1].split(" s,")[0])
                    series[route].append({"survey_s": secs, "process_s": wall})
                    lines[route] = [l for l in r.stdout.splitlines() if l.startswith("survey")]
                    reports.add(open(rep_file, "rb").read())
            med = {k: statistics.median(x["survey_s"] for x in v) for k, v in series.items()}
            out[kind] = {"runs": series, "survey_s_median": med, "frames_per_s": {k: n / v for k, v in med.items()},
                         "gpu_over_host": med["host"] / med["gpu"], "last_lines": lines}
        out["reports_identical"] = len(reports) == 1
        out["run_line"] = reports.pop().decode().splitlines()[-1]
        out["frames"] = n
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def part_e():
    """the committed sample frame of the 40l-19 data as a one-event run: the one real frame three times over (the Trainer
    wants two frames, the pairing a third), surveyed on both routes -> the report's model and run lines"""
    run_id = "20200925_0"
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    sample = os.path.join(ROOT, "tests", "golden", "sample_40l19_cam1_image30.png")
    tmp = tempfile.mkdtemp(prefix="abub_survey_sample_")
    try:
        d = os.path.join(tmp, run_id, "0", "Images")
        os.makedirs(d)
        for k in range(3):
            shutil.copy(sample, os.path.join(d, f"cam1_image{30 + k}.png"))
        texts = []
        for flag in ([], ["--survey-gpu"]):
            rep = os.path.join(tmp, "report.txt")
            r = subprocess.run([exe, "-d", tmp, "-r", run_id, "-D", "40l-19", "--survey", rep] + flag, env=dict(os.environ, ABUB_NUM_CAMS="2"),
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            texts.append(open(rep).read())
        assert texts[0] == texts[1]
        return {"frames": 3, "routes_identical": True, "report": texts[0].splitlines()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def part_d(parent, balanced):
    """balanced: an order such as TPPTTPPTTPPT (tools/verify_bench.py part_c_balanced) instead of the three pairs"""
    import abf_bench
    import verify_bench

    return verify_bench.part_c_balanced(parent, balanced) if balanced else abf_bench.part_c(parent)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abcde")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "survey.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--balanced", nargs="?", const="TPPTTPPTTPPT", default=None)
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):  # (a call that measures some of the parts keeps the others)
        result = json.load(open(a.out))
    for part, fn in (("a", lambda: part_a(a.frames)), ("b", lambda: part_b(a.frames)), ("c", lambda: part_c(a.frames)),
                     ("e", part_e), ("d", lambda: part_d(a.parent, a.balanced))):
        key = {"a": "kernel", "b": "host_definition", "c": "end_to_end", "d": "parent_comparison_" + a.balanced if a.balanced else "parent_comparison", "e": "sample_frame_run"}[part]
        if part not in a.parts or (part == "d" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
