#!/usr/bin/env python3
"""A campaign of synthetic runs through the CLI, timed three ways, alternately: (a) one abub3hs process per run, in sequence;
(b) one process with --run-list; (c) (b) with ABUB_TRAIN_ON_GPU=0 (the host Trainer).  Every process runs under
`timeout -k 10`, and the tool stops at the first nonzero exit.  The three must write byte-identical files.  Also times the
training of one run on the device (Run.train_on_gpu) against the host Trainer (Run.train per camera).
usage: python3 tools/campaign_bench.py [--runs 4] [--events 32] [--reps 3] [--out profiles/r04/campaign.json]"""
import argparse, hashlib, io, json, os, re, shutil, statistics, subprocess, sys, tempfile, time, zipfile
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from concurrent.futures import ThreadPoolExecutor
from PIL import Image
from autobub3hs_amd import host, synth

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
EXE = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=4)
ap.add_argument("--events", type=int, default=32)
ap.add_argument("--width", type=int, default=1280)
ap.add_argument("--height", type=int, default=1024)
ap.add_argument("--frames", type=int, default=41)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--timeout", type=int, default=300, help="seconds per CLI process")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r04", "campaign.json"))
a = ap.parse_args()
W, H, F, E, C, R = a.width, a.height, a.frames, a.events, 2, a.runs
ids = ["20200925_%d" % r for r in range(R)]
ENV = dict(os.environ, ABUB_NUM_CAMS=str(C))


def write_run(tmp, r, run_id):
    def enc(job):
        e, c = job
        seed = 1000 * (r + 1) + e
        st = synth.render_event(W, H, synth.random_spec(W, H, F, seed, c, p_second=0.2), seed, c)
        out = []
        for k in range(F):
            b = io.BytesIO()
            Image.fromarray(st[k]).save(b, format="PNG", compress_level=1)
            out.append((e, c, k, b.getvalue()))
        return out

    with ThreadPoolExecutor(min(16, len(os.sched_getaffinity(0)))) as ex:
        blobs = [x for l in ex.map(enc, [(e, c) for e in range(E) for c in range(C)]) for x in l]
    with zipfile.ZipFile(os.path.join(tmp, run_id + ".zip"), "w", zipfile.ZIP_STORED) as z:
        for e in range(E):
            z.writestr(f"{run_id}/{e}/", b"")
            z.writestr(f"{run_id}/{e}/Images/", b"")
        for e, c, k, data in blobs:
            z.writestr(f"{run_id}/{e}/Images/cam{c}_image{30 + k}.png", data)


def cli(args, env):
    t0 = time.perf_counter()
    p = subprocess.run(["timeout", "-k", "10", str(a.timeout), EXE] + args, capture_output=True, text=True, env=env)
    dt = time.perf_counter() - t0
    if p.returncode != 0:
        print(p.stdout[-3000:], p.stderr[-3000:], file=sys.stderr)
        sys.exit(f"abub3hs exited with {p.returncode}: {' '.join(args)}")
    return dt, p.stdout


def digest(out):
    return {r: hashlib.sha256(open(os.path.join(out, f"abub3hs_{r}.txt"), "rb").read()).hexdigest()[:16] for r in ids}


tmp = tempfile.mkdtemp(prefix="abub_campaign_")
try:
    t0 = time.perf_counter()
    for r, rid in enumerate(ids):
        write_run(tmp, r, rid)
    mb = sum(os.path.getsize(os.path.join(tmp, r + ".zip")) for r in ids) / 1e6
    sizes = {"runs": R, "events_per_run": E, "cams": C, "frames_per_stack": F, "W": W, "H": H, "archive": "zip (stored PNG)",
             "frames_total": R * E * C * F, "archives_MB": round(mb), "write_s": round(time.perf_counter() - t0, 1)}
    print(json.dumps(sizes), flush=True)
    lst = os.path.join(tmp, "runs.txt")
    open(lst, "w").write("\n".join(ids) + "\n")
    modes = {"a_process_per_run": [], "b_run_list": [], "c_run_list_host_training": []}
    digests = {}
    for rep in range(a.reps):
        for mode in modes:
            out = os.path.join(tmp, f"out_{mode}_{rep}")
            os.makedirs(out)
            base = ["-z", "-d", tmp, "-o", out, "-D", "40l-19"]
            if mode == "a_process_per_run":
                dt = sum(cli(base + ["-r", r], ENV)[0] for r in ids)
                rec = {"wall_s": round(dt, 3)}
            else:
                env = dict(ENV, ABUB_TRAIN_ON_GPU="0" if mode.startswith("c") else "1")
                dt, so = cli(base + ["--run-list", lst], env)
                m = re.search(r"campaign: .*training ([\d.]+) s \(exposed ([\d.]+) s\); pipelines built (\d+)", so)
                rec = {"wall_s": round(dt, 3), "training_s": float(m.group(1)), "training_exposed_s": float(m.group(2)),
                       "pipelines_built": int(m.group(3))}
            rec["frames_per_s"] = round(R * E * C * F / dt)
            modes[mode].append(rec)
            digests.setdefault(mode, digest(out))
            assert digest(out) == digests[mode], f"{mode}: output differs between repetitions"
            print(json.dumps({"rep": rep, "mode": mode, **rec}), flush=True)
    identical = digests["a_process_per_run"] == digests["b_run_list"] == digests["c_run_list_host_training"]
    assert identical, digests
    # training of one run: device (one pass, every camera) against the host Trainer (camera by camera)
    run = host.Run(kind="zip", run_folder=os.path.join(tmp, ids[0]))
    train = {"device_s": [], "host_s": []}
    for rep in range(a.reps):
        t1 = time.perf_counter()
        dev = run.train_on_gpu(C, shape=(H, W))
        train["device_s"].append(round(time.perf_counter() - t1, 3))
        assert run.train_path == "device" and run.train_stats["frames_gpu_decoded"] == 2 * E * C, run.train_stats
        train["device_stats"] = run.train_stats
        t1 = time.perf_counter()
        hst = [run.train(c, shape=(H, W)) for c in range(C)]
        train["host_s"].append(round(time.perf_counter() - t1, 3))
        assert all(d[0] == h[0] == 0 and d[1] == h[1] and (d[2] == h[2]).all() and (d[3] == h[3]).all() for d, h in zip(dev, hst))
    run.close()
    summary = {}
    for mode, recs in modes.items():
        w = [r["wall_s"] for r in recs]
        summary[mode] = {"wall_s_median": round(statistics.median(w), 3), "wall_s_min": min(w), "wall_s_max": max(w),
                         "frames_per_s_median": round(R * E * C * F / statistics.median(w))}
        for k in ("training_s", "training_exposed_s", "pipelines_built"):
            if k in recs[0]:
                summary[mode][k + "_median"] = statistics.median(r[k] for r in recs)
    summary["speedup_b_over_a"] = round(summary["a_process_per_run"]["wall_s_median"] / summary["b_run_list"]["wall_s_median"], 3)
    result = {"sizes": sizes, "reps": a.reps, "runs": modes, "summary": summary, "outputs_identical": identical,
              "output_sha256_16": digests["b_run_list"],
              "train_one_run": {**train, "device_s_median": statistics.median(train["device_s"]),
                                "host_s_median": statistics.median(train["host_s"])}}
    print(json.dumps(result["summary"]), flush=True)
    print(json.dumps(result["train_one_run"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
finally:
    shutil.rmtree(tmp, ignore_errors=True)
