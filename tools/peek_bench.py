#!/usr/bin/env python3
"""abub_peek_planes_dev measured on one GPU box, in one call -> profiles/r18/peek.json.
  (a) kernel: 1024 resident 1280x1024 items (D planes and trigger frames in slabs, item i at i * W * H, three rectangles
      each) against a device-to-device copy of the same bytes (2 * W * H read and 2 * W * H written per item: two
      hipMemcpyAsync calls, one per slab), alternating five times each, device events, medians.  The copy is the
      yardstick; no ratio is fixed in advance.  Checked first: every plane of the launch against numpy on the device.
  (d) parent comparison: tools/abf_bench.py part (c) (bench.py --steps 20 --warmup 5, parent build and this tree
      alternating, three runs each, dumped outputs compared byte for byte); --balanced [ORDER]: tools/verify_bench.py's
      twelve-run order instead.
  (b) end to end: the archive of tools/ingest_bench.py (--events of them, a stored PNG zip, 1280x1024, 2 cameras, 41
      frames) through Run.run_batched without peek, with peek on the GPU route and with peek on the host route
      (ABUB_PEEK_GPU=0), three alternating repetitions, medians; the files of the two routes compared byte for byte;
  (c) the per-event loop's write-out: abub3hs --debug 100 on the first --debug-events events of the same run, written out
      as a directory (a stated subset: the loop decodes every frame on host threads and writes with zlib), against
      abub3hs --peek on the same directory;
usage: python3 tools/peek_bench.py [--parts abcd] [--parent DIR] [--balanced [ORDER]] [--out profiles/r18/peek.json] [--items 1024]
       [--events 96] [--debug-events 8]"""
import argparse, filecmp, io, json, os, shutil, statistics, subprocess, sys, tempfile, time, zipfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402


def part_a(n, W=1280, H=1024):
    import torch
    from autobub3hs_amd import hip, synth, _lib

    F = 41
    P = W * H
    dev = torch.device("cuda:0")
    fr = np.asarray(synth.render_event(W, H, synth.random_spec(W, H, F, 3, 0), 3, 0))
    pick = torch.arange(n, device=dev) % F
    frames = torch.from_numpy(fr).to(dev)[pick].contiguous().reshape(-1)
    diff = (frames.reshape(n, P) - frames.reshape(n, P).roll(1, dims=0)).reshape(-1)  # (wrapping u8 differences: any bytes do)
    out = torch.empty(2 * n * P, dtype=torch.uint8, device=dev)
    thr = 3 + np.arange(n) % 5
    rects = np.array([(100 + 7 * (i % 50), 200 + 3 * (i % 90), 40 + i % 30, 25 + i % 40) for i in range(3 * n)], np.int32)
    rows = [(i * P, i * P, 2 * i * P, (2 * i + 1) * P, int(thr[i]), 3 * i, 3) for i in range(n)]
    d_items = torch.from_numpy(hip.peek_items(rows)).to(dev)
    d_rects = torch.from_numpy(rects).to(dev)
    status = torch.full((n,), 99, dtype=torch.int32, device=dev)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def go():
        _lib.check(L.abub_peek_planes_dev(diff.data_ptr(), diff.numel(), frames.data_ptr(), frames.numel(), d_items.data_ptr(), n,
                                          d_rects.data_ptr(), len(rects), W, H, out.data_ptr(), out.numel(), status.data_ptr(), stream),
                   "peek")

    def copy():
        o = out.reshape(n, 2, P)
        o[:, 0].copy_(diff.reshape(n, P))  # (strided destination: torch launches its own copy kernel)
        o[:, 1].copy_(frames.reshape(n, P))

    flat = torch.empty(2 * n * P, dtype=torch.uint8, device=dev)

    def copy_flat():  # the same bytes as two contiguous device-to-device memcpys
        flat[:n * P].copy_(diff)
        flat[n * P:].copy_(frames)

    go()
    torch.cuda.synchronize()
    assert not status.any().item()
    o = out.reshape(n, 2, H, W)
    exp_thr = (diff.reshape(n, H, W) > torch.from_numpy(thr.astype(np.uint8)).to(dev)[:, None, None]).to(torch.uint8) * 255
    assert torch.equal(o[:, 0], exp_thr)
    drawn = (o[:, 1] != frames.reshape(n, H, W))
    assert bool((o[:, 1][drawn] == 255).all())
    import importlib.util
    spec = importlib.util.spec_from_file_location("peekref", os.path.join(ROOT, "tests", "peekref.py"))
    peekref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(peekref)
    for i in (0, n // 2, n - 1):  # the drawn frames of three items, pixel for pixel
        want = peekref.presentation(frames.reshape(n, H, W)[i].cpu().numpy(), rects[3 * i:3 * i + 3])
        assert np.array_equal(o[i, 1].cpu().numpy(), want), i

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for fn in (go, copy, copy_flat):
        fn()
    torch.cuda.synchronize()
    t = {"kernel": [], "copy_strided": [], "copy_flat": []}
    for _ in range(5):
        t["kernel"].append(timed(go))
        t["copy_strided"].append(timed(copy))
        t["copy_flat"].append(timed(copy_flat))
    med = {k: statistics.median(v) for k, v in t.items()}
    moved = 4 * n * P  # read 2 planes, write 2 planes
    return {"items": n, "W": W, "H": H, "rects_per_item": 3, "bytes_read_plus_written": moved, "ms": t, "ms_median": med,
            "TBps": {k: moved / v / 1e9 for k, v in med.items()}, "items_per_s": n / med["kernel"] * 1e3,
            "kernel_over_copy_flat": med["kernel"] / med["copy_flat"], "kernel_over_copy_strided": med["kernel"] / med["copy_strided"]}


def part_bc(E, Edbg, W=1280, H=1024, F=41, C=2):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from autobub3hs_amd import host, synth

    run_id = "20200925_0"
    tmp = tempfile.mkdtemp(prefix="abub_peek_")
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
        with zipfile.ZipFile(os.path.join(tmp, run_id + ".zip"), "w", zipfile.ZIP_STORED) as z:
            for e in range(E):
                z.writestr(f"{run_id}/{e}/", b"")
                z.writestr(f"{run_id}/{e}/Images/", b"")
            for e, c, k, data in blobs:
                z.writestr(f"{run_id}/{e}/Images/cam{c}_image{30 + k}.png", data)
        for e, c, k, data in blobs:  # the subset of part (c), as a directory
            if e < Edbg:
                d = os.path.join(tmp, "dir", run_id, str(e), "Images")
                os.makedirs(d, exist_ok=True)
                with open(os.path.join(d, f"cam{c}_image{30 + k}.png"), "wb") as f:
                    f.write(data)
        del blobs
        print("peek_bench: archive written", flush=True)
        run = host.Run(kind="zip", run_folder=os.path.join(tmp, run_id))
        assert all(run.train(c, shape=(H, W))[0] == 0 for c in range(C))
        res = {"plain": [], "peek_gpu": [], "peek_host": []}
        text = {}
        for rep in range(3):
            for tag in res:
                out = os.path.join(tmp, f"out_{tag}{rep}") + "/"
                os.makedirs(out)
                peek = None if tag == "plain" else os.path.join(tmp, f"{tag}{rep}")
                os.environ["ABUB_PEEK_GPU"] = "0" if tag == "peek_host" else "1"
                t0 = time.perf_counter()
                st = run.run_batched(C, out, run_id, 30, nthreads=16, decode_threads=16, peek_dir=peek)
                dt = time.perf_counter() - t0
                os.environ.pop("ABUB_PEEK_GPU", None)
                text[tag] = open(os.path.join(out, f"abub3hs_{run_id}.txt")).read()
                row = {"seconds": dt, "frames_per_s": E * C * F / dt, "gpu_s": st["gpu_s"]}
                if peek:
                    row.update({k: st[k] for k in ("peek_stacks", "peek_files", "peek_bytes", "peek_gpu", "peek_s")})
                res[tag].append(row)
                print(f"peek_bench: {tag} {rep}: {row['frames_per_s']:.0f} frames/s" + (f", peek {st['peek_s']:.3f} s" if peek else ""), flush=True)
        run.close()
        a, b = os.path.join(tmp, "peek_gpu0", run_id), os.path.join(tmp, "peek_host0", run_id)
        names = sorted(os.listdir(a))
        same = names == sorted(os.listdir(b)) and len(names) > 0 and all(filecmp.cmp(os.path.join(a, n), os.path.join(b, n), shallow=False) for n in names)
        med = {t: statistics.median(r["frames_per_s"] for r in res[t]) for t in res}
        end_to_end = {"events": E, "frames": E * C * F, "source": "stored PNG zip", "runs": res, "median_frames_per_s": med,
                      "median_peek_s": {t: statistics.median(r["peek_s"] for r in res[t]) for t in ("peek_gpu", "peek_host")},
                      "peek_gpu_over_plain": med["peek_gpu"] / med["plain"], "peek_host_over_plain": med["peek_host"] / med["plain"],
                      "files": len(names), "routes_write_identical_files": same,
                      "same_text_with_and_without_peek": text["plain"] == text["peek_gpu"] == text["peek_host"]}
        # (c) the per-event loop with its write-out against --peek, on the first Edbg events as a directory
        exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
        rows = {}
        for tag, args in (("debug_100", ["--debug", "100"]), ("peek", ["--peek", os.path.join(tmp, "cli_peek")])):
            out = os.path.join(tmp, "cli_" + tag + "_out")
            os.makedirs(out)
            os.makedirs(os.path.join(tmp, "DebugPeek"), exist_ok=True)
            t0 = time.perf_counter()
            p = subprocess.run([exe, "-d", os.path.join(tmp, "dir"), "-r", run_id, "-o", out, "-D", "40l-19"] + args, capture_output=True,
                               text=True, env=dict(os.environ, ABUB_NUM_CAMS=str(C), ABUB_THREADS="16"), cwd=tmp, timeout=900)
            assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
            rows[tag] = {"seconds": time.perf_counter() - t0, "text": open(os.path.join(out, f"abub3hs_{run_id}.txt")).read()}
            print(f"peek_bench: abub3hs {' '.join(args[:1])}: {rows[tag]['seconds']:.2f} s", flush=True)
        per_event = {"events": Edbg, "frames": Edbg * C * F, "source": "directory of PNG files, the first events of the run above",
                     "process_seconds": {t: rows[t]["seconds"] for t in rows}, "same_text": rows["debug_100"]["text"] == rows["peek"]["text"],
                     "debug_files": len(os.listdir(os.path.join(tmp, "DebugPeek"))),
                     "peek_files": len(os.listdir(os.path.join(tmp, "cli_peek", run_id)))}
        return end_to_end, per_event
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--events", type=int, default=96)
    ap.add_argument("--debug-events", type=int, default=8)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--balanced", nargs="?", const="TPPTTPPTTPPT", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "peek.json"))
    ap.add_argument("--items", type=int, default=1024)
    a = ap.parse_args()

    def part_d():
        import abf_bench
        import verify_bench

        return verify_bench.part_c_balanced(a.parent, a.balanced) if a.balanced else abf_bench.part_c(a.parent)

    result = {}
    if os.path.exists(a.out):  # (a second call adds to the first)
        result = json.load(open(a.out))
    for k in ("run_batched_with_and_without_peek", "per_event_debug_100"):
        if isinstance(result.get(k), str):
            del result[k]

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)

    if "b" in a.parts or "c" in a.parts:
        result["end_to_end"], result["per_event_debug_100"] = part_bc(a.events, min(a.debug_events, a.events))
        print(json.dumps({"end_to_end": result["end_to_end"], "per_event_debug_100": result["per_event_debug_100"]}), flush=True)
        save()
    else:
        result.setdefault("end_to_end", "not measured")
        result.setdefault("per_event_debug_100", "not measured")
    for part, fn in (("a", lambda: part_a(a.items)), ("d", part_d)):
        key = {"a": "kernel", "d": "parent_comparison_" + a.balanced if a.balanced else "parent_comparison"}[part]
        if part not in a.parts or (part == "d" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
