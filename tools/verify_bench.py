#!/usr/bin/env python3
"""abub_frames_compare_dev and abub3hs --verify-repack [--verify-gpu] measured on one GPU box, in one call ->
profiles/r11/verify.json.
  (a) kernel: 1024 pairs of resident 1280x1024 synth frames, identical, against the same pairs with 1 % of the bytes
      differing (what the slow path costs), alternating five times each, device events, medians; bytes read per second
      (2 * W * H per pair); the same bytes through the read mode of tools/rowload_bench (read_guide, the shape that holds the
      read ceiling of DESIGN section 6), run in the same call; the ratio of the two;
  (b) end to end: the 96-event archive of tools/ingest_bench.py (a stored PNG zip), repacked once; Run.verify on 16 threads
      against Run.verify(device=0), three alternating repetitions, medians, and the legs of the device route (read, upload +
      decode, compare) summed over its batches;
  (c) parent comparison: tools/abf_bench.py part (c) (bench.py --steps 20 --warmup 5, parent build and this tree
      alternating, three runs each, dumped outputs compared byte for byte); --balanced [ORDER]: twelve runs in the balanced
      order T P P T ... of DESIGN section 3 instead (or in ORDER, e.g. its mirror image PTTPPTTPPTTP).
usage: python3 tools/verify_bench.py [--parts abc] [--parent DIR] [--balanced [ORDER]] [--out profiles/r11/verify.json] [--pairs 1024] [--events 96]"""
import argparse, filecmp, io, json, os, shutil, statistics, subprocess, sys, tempfile, zipfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402


def rowload_read(frames):
    """the read mode of tools/rowload_bench over `frames` 1280x1024 frames -> its "guide read" lines"""
    exe = os.path.join(ROOT, "tools", "rowload_bench")
    if not os.path.exists(exe):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", exe + ".cpp", "-o", exe])
    r = subprocess.run([exe, str(frames), "0", "copy"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and '"guide read"' in l]


def part_a(n, W=1280, H=1024):
    import torch
    from autobub3hs_amd import hip, synth, _lib

    F = 41
    spec = synth.random_spec(W, H, F, 3, 0)
    fr = np.asarray(synth.render_event(W, H, spec, 3, 0))
    P = W * H
    dev = torch.device("cuda:0")
    a = torch.from_numpy(fr).to(dev)[torch.arange(n, device=dev) % F].contiguous().reshape(-1)
    b, c = a.clone(), a.clone()  # b: identical; c: 1 % of the bytes differ
    want = np.zeros(n, np.int64)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for f0 in range(0, n, 32):
        part = c[f0 * P:min(n, f0 + 32) * P]
        hit = torch.rand(part.numel(), device=dev, generator=g) < 0.01
        part[hit] ^= 0x5A
        want[f0:f0 + 32] = hit.reshape(-1, P).sum(dim=1).cpu().numpy()
    pairs = np.stack([np.arange(n, dtype=np.int64) * P] * 2, axis=1)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    d_pairs = torch.from_numpy(pairs).to(dev)
    res = torch.empty((n, 4), dtype=torch.int32, device=dev)
    got = hip.frames_compare(a, b, pairs, P)
    assert (got[:, 0] == 0).all() and (got[:, 1] == 0).all() and (got[:, 2] == 0xFFFFFFFF).all() and (got[:, 3] == 0).all()
    got = hip.frames_compare(a, c, pairs, P)
    assert (got[:, 0] == 0).all() and np.array_equal(got[:, 1], want) and (got[:, 3] > 0).all()

    def go(other):
        _lib.check(L.abub_frames_compare_dev(a.data_ptr(), a.numel(), other.data_ptr(), other.numel(), d_pairs.data_ptr(), n, P,
                                             res.data_ptr(), stream), "cmp")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    go(b)
    torch.cuda.synchronize()
    t_same, t_diff = [], []
    for _ in range(5):
        t_same.append(timed(lambda: go(b)))
        t_diff.append(timed(lambda: go(c)))
    del b, c
    torch.cuda.empty_cache()
    ms, ms_diff, nbytes = statistics.median(t_same), statistics.median(t_diff), 2 * n * P
    lines = rowload_read(2 * n)
    best = max(l["TBps"] for l in lines)
    return {"pairs": n, "W": W, "H": H, "bytes_read": nbytes, "identical_ms": t_same, "one_percent_differing_ms": t_diff,
            "identical_ms_median": ms, "identical_TBps": nbytes / ms / 1e9, "pairs_per_s": n / ms * 1e3,
            "one_percent_differing_ms_median": ms_diff, "one_percent_differing_TBps": nbytes / ms_diff / 1e9,
            "slow_path_over_fast_path": ms_diff / ms, "rowload_bench_guide_read": lines, "rowload_bench_read_TBps": best,
            "kernel_over_rowload_read": nbytes / ms / 1e9 / best}


def part_b(E, W=1280, H=1024, F=41, C=2):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from autobub3hs_amd import host, synth

    run_id = "20200925_0"
    tmp = tempfile.mkdtemp(prefix="abub_verify_")
    try:
        def enc(job):
            e, c = job
            st = synth.render_event(W, H, synth.random_spec(W, H, F, e, c, p_second=0.2), e, c)
            out = []
            for k in range(F):
                b = io.BytesIO()
                Image.fromarray(st[k]).save(b, format="PNG", compress_level=1)
                out.append((e, c, k, b.getvalue()))
            return out

        with ThreadPoolExecutor(min(16, len(os.sched_getaffinity(0)))) as ex:
            blobs = [x for l in ex.map(enc, [(e, c) for e in range(E) for c in range(C)]) for x in l]
        os.makedirs(os.path.join(tmp, "png"))
        with zipfile.ZipFile(os.path.join(tmp, "png", run_id + ".zip"), "w", zipfile.ZIP_STORED) as z:
            for e in range(E):
                z.writestr(f"{run_id}/{e}/", b"")
                z.writestr(f"{run_id}/{e}/Images/", b"")
            for e, c, k, data in blobs:
                z.writestr(f"{run_id}/{e}/Images/cam{c}_image{30 + k}.png", data)
        del blobs
        print("verify_bench: archive written", flush=True)
        src = host.Run(kind="zip", run_folder=os.path.join(tmp, "png", run_id))
        packed = os.path.join(tmp, "packed", run_id)
        st = src.repack(packed, nthreads=16, ncams=C, device=0)
        assert st["packed"] == E * C * F and st["failed"] == 0
        print("verify_bench: repacked", flush=True)
        other = host.Run(kind="raw", run_folder=packed + "/")
        res = {"host": [], "gpu": []}
        for rep in range(3):
            for tag, device in (("host", None), ("gpu", 0)):
                r = src.verify(other, nthreads=16, ncams=C, device=device)
                assert r["rc"] == 0 and r["same"] == E * C * F == r["frames"] and not r["findings"], r
                assert device is None or (r["device"] == 0 and r["frames_kernel"] == r["frames"])
                res[tag].append(dict({k: v for k, v in r.items() if k != "findings"}, frames_per_s=r["frames"] / r["seconds"]))
                print(f"verify_bench: {tag} {rep}: {res[tag][-1]['frames_per_s']:.0f} frames/s", flush=True)
        src.close()
        other.close()
        med = {t: statistics.median(r["frames_per_s"] for r in res[t]) for t in res}
        legs = ("read_s", "decode_s", "compare_s", "seconds")
        return {"events": E, "frames": E * C * F, "source": "stored PNG zip", "copy": "directory of packed frames",
                "runs": res, "median_frames_per_s": med, "gpu_over_host": med["gpu"] / med["host"],
                "gpu_route_legs_s_median": {k: statistics.median(r[k] for r in res["gpu"]) for k in legs},
                "gpu_route_batches": int(res["gpu"][0]["batches"])}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def part_c_balanced(parent, order):
    """one run per letter of `order` (T: this tree, P: the parent build), e.g. T P P T T P P T T P P T (six each)"""
    import abf_bench

    tmp = tempfile.mkdtemp(prefix="abub_verify_ab_")
    try:
        series, dumps = {"parent": [], "tree": []}, {"parent": [], "tree": []}
        for i, who in enumerate(order):
            who = "tree" if who == "T" else "parent"
            dumps[who].append(os.path.join(tmp, f"{who}{i}"))
            res = abf_bench.bench_once(ROOT if who == "tree" else parent, dumps[who][-1])
            series[who].append({"value": res["value"], "ms_per_step": res.get("ms_per_step")})
            print(f"verify_bench: {who}: {res['value']:.0f}", flush=True)
        names = sorted(os.listdir(dumps["parent"][0]))
        same = len(names) > 0 and all(sorted(os.listdir(d)) == names and
                                      all(filecmp.cmp(os.path.join(dumps["parent"][0], f), os.path.join(d, f), shallow=False) for f in names)
                                      for d in dumps["parent"] + dumps["tree"])
        med = {k: statistics.median(r["value"] for r in v) for k, v in series.items()}
        return {"command": "bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR", "order": " ".join(order), "runs": series,
                "median_frames_per_s": med, "tree_over_parent": med["tree"] / med["parent"], "dumped_outputs_identical": same}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--balanced", nargs="?", const="TPPTTPPTTPPT", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "verify.json"))
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--events", type=int, default=96)
    a = ap.parse_args()

    def part_c():
        import abf_bench

        return part_c_balanced(a.parent, a.balanced) if a.balanced else abf_bench.part_c(a.parent)

    result = {}
    if os.path.exists(a.out):  # (a second call adds to the first: the balanced series next to the three pairs)
        result = json.load(open(a.out))
    for part, fn in (("a", lambda: part_a(a.pairs)), ("b", lambda: part_b(a.events)), ("c", part_c)):
        key = {"a": "kernel", "b": "end_to_end", "c": "parent_comparison_" + a.balanced if a.balanced else "parent_comparison"}[part]
        if part not in a.parts or (part == "c" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
