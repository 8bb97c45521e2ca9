#!/usr/bin/env python3
"""The packed frame format ("ABF1") measured on one GPU box, in one call -> profiles/r09/abf.json.
  (a) kernel: abub_abf_decode_dev over 1024 resident packed 1280x1024 frames against abub_png_decode_dev over the same
      frames as level-1 PNGs (made like tools/png_bench.py makes them), alternating five times each, device events;
  (b) end to end: the 96-event archive of tools/ingest_bench.py as a stored PNG zip, and its repacked copy as a directory
      and as a stored zip, through RunBatched with the default settings, three alternating repetitions, with the PNG zip
      also through a built checkout of the parent commit and, the same way, through this tree (--parent DIR; one process
      per repetition and build); the repack's own rate; the worker timeline (ABUB_INGEST_TRACE=1) of one more packed run;
  (c) parent comparison: `python bench.py --steps 20 --warmup 5 --dump-outputs DIR` in a built checkout of the parent
      commit (--parent DIR) and in this tree, alternating, three runs each; outputs compared byte for byte.
usage: python3 tools/abf_bench.py [--parts abc] [--parent DIR] [--out profiles/r09/abf.json] [--frames 1024] [--events 96]"""
import argparse, filecmp, io, json, os, shutil, statistics, subprocess, sys, tempfile, time, zipfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.environ.get("ABUB_BENCH_TREE") or ROOT)  # (the package of another checkout: the parent's PNG path)
import numpy as np  # noqa: E402

READ_CEILING_TBPS, FILL_CEILING_TBPS = 6.14, 5.95  # DESIGN section 6 (profiles/r03/copy_ceiling.jsonl)


def part_a(n, W=1280, H=1024):
    import torch
    from PIL import Image
    from autobub3hs_amd import hip, host, synth, _lib

    F = 41
    spec = synth.random_spec(W, H, F, 3, 0)
    fr = np.asarray(synth.render_event(W, H, spec, 3, 0))
    P = W * H
    png, abf = [], []
    for k in range(F):
        b = io.BytesIO()
        Image.fromarray(fr[k]).save(b, format="PNG", compress_level=1)
        png.append(b.getvalue())
        abf.append(host.abf_encode(fr[k]))
    dev = torch.device("cuda:0")
    # ---- packed: files at 16-byte-rounded offsets, frame i at i * P
    blob, descs = bytearray(), []
    for i in range(n):
        descs.append((len(blob), len(abf[i % F]), i * P))
        blob += abf[i % F]
        blob += b"\0" * (-len(blob) % 16)
    a_files = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
    rec = np.zeros((n, 4), np.uint32)
    rec[:, 0], rec[:, 1] = [d[0] for d in descs], [d[1] for d in descs]
    rec[:, 2], rec[:, 3] = [d[2] & 0xFFFFFFFF for d in descs], [d[2] >> 32 for d in descs]
    a_desc = torch.from_numpy(rec.view(np.int32).copy()).to(dev)
    a_status = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    # ---- PNG: as tools/png_bench.py
    frames_np = np.zeros((n, 8), dtype=np.uint32)
    segs, pblob, zoff = [], bytearray(), 0
    for i in range(n):
        data = png[i % F]
        sg, lut = hip.png_parse(data, W, H)
        base, zlen = len(pblob), sum(l for _, l in sg)
        frames_np[i] = (len(segs), len(sg), zoff, zlen, 0xFFFFFFFF, 0, (i * P) & 0xFFFFFFFF, (i * P) >> 32)
        segs += [(base + o, l) for o, l in sg]
        pblob += data
        pblob += b"\0" * ((-len(pblob)) % 4)
        zoff += ((zlen + 15) & ~15) + 16
    pblob += b"\0" * 8
    p_files = torch.frombuffer(pblob, dtype=torch.uint8).to(dev)
    p_frames = torch.from_numpy(frames_np.view(np.int32).copy()).to(dev)
    p_segs = torch.tensor(segs, dtype=torch.int64).to(torch.int32).to(dev)
    p_luts = torch.zeros(256, dtype=torch.uint8, device=dev)
    stride = int(_lib.lib().abub_png_raw_stride(W, H))
    p_z = torch.empty((zoff,), dtype=torch.uint8, device=dev)
    p_raw = torch.empty((n * stride,), dtype=torch.uint8, device=dev)
    p_status = torch.zeros(n, dtype=torch.int32, device=dev)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def go_abf():
        _lib.check(L.abub_abf_decode_dev(a_files.data_ptr(), a_files.numel(), a_desc.data_ptr(), n, W, H, out.data_ptr(),
                                         out.numel(), a_status.data_ptr(), stream), "abf")

    def go_png():
        _lib.check(L.abub_png_decode_dev(p_files.data_ptr(), p_files.numel(), p_frames.data_ptr(), n, p_segs.data_ptr(), len(segs),
                                         p_luts.data_ptr(), 0, W, H, p_z.data_ptr(), p_z.numel(), p_raw.data_ptr(), p_raw.numel(),
                                         out.data_ptr(), out.numel(), p_status.data_ptr(), stream), "png")

    def check(status):
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all()
        for k in range(0, n, max(1, n // 7)):
            assert np.array_equal(out[k].cpu().numpy(), fr[k % F]), k
        out.zero_()

    go_abf()
    check(a_status)
    go_png()
    check(p_status)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    t_abf, t_png = [], []
    for _ in range(5):
        t_abf.append(timed(go_abf))
        t_png.append(timed(go_png))
    ms = statistics.median(t_abf)
    file_bytes = sum(d[1] for d in descs)
    moved = file_bytes + n * P
    floor_ms = (file_bytes / READ_CEILING_TBPS + n * P / FILL_CEILING_TBPS) / 1e9
    return {"frames": n, "W": W, "H": H, "packed_MB_per_frame": file_bytes / n / 1e6, "png_MB_per_frame": len(pblob) / n / 1e6,
            "abf_ms": t_abf, "png_ms": t_png, "abf_ms_median": ms, "png_ms_median": statistics.median(t_png),
            "abf_frames_per_s": n / ms * 1e3, "png_frames_per_s": n / statistics.median(t_png) * 1e3,
            "abf_bytes_read_plus_written": moved, "abf_TBps": moved / ms / 1e9,
            "share_of_read_ceiling": moved / ms / 1e9 / READ_CEILING_TBPS, "share_of_fill_ceiling": moved / ms / 1e9 / FILL_CEILING_TBPS,
            "floor_ms_one_read_one_write": floor_ms, "times_above_floor": ms / floor_ms,
            "packed_faster_than_png": ms < statistics.median(t_png)}


def zip_dir(rd, path):
    root = os.path.dirname(rd)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED, allowZip64=True) as z:
        for dp, dn, fn in os.walk(rd):
            rel = os.path.relpath(dp, root)
            z.writestr(rel + "/", b"")
            for f in sorted(fn):
                z.write(os.path.join(dp, f), os.path.join(rel, f))


def png_run(where, shape, frames):
    """one RunBatched of a PNG archive with whatever package sys.path gives (this tree's, or ABUB_BENCH_TREE's) -> a JSON line"""
    from autobub3hs_amd import host

    W, H, C = (int(x) for x in shape.split("x"))
    run = host.Run(kind="zip", run_folder=where)
    assert all(run.train(c, shape=(H, W))[0] == 0 for c in range(C))
    tmp = tempfile.mkdtemp(prefix="abub_abf_png_")
    try:
        t0 = time.perf_counter()
        st = run.run_batched(C, tmp + "/", "p", 30)
        dt = time.perf_counter() - t0
        text = open(os.path.join(tmp, "abub3hs_p.txt")).read()
    finally:
        run.close()
        shutil.rmtree(tmp, ignore_errors=True)
    import hashlib
    print(json.dumps({"s": dt, "frames_per_s": frames / dt, "decode_s": st["decode_s"], "gpu_s": st["gpu_s"],
                      "gpudecode_s": st["gpudecode_s"], "frames_gpu_decoded": int(st["frames_gpu_decoded"]),
                      "text_sha1": hashlib.sha1(text.encode()).hexdigest()}), flush=True)


def part_b(E, parent=None, W=1280, H=1024, F=41, C=2):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from autobub3hs_amd import host, synth

    run_id = "20200925_0"
    tmp = tempfile.mkdtemp(prefix="abub_abf_")
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
        zpng = os.path.join(tmp, "png", run_id + ".zip")
        with zipfile.ZipFile(zpng, "w", zipfile.ZIP_STORED) as z:
            for e in range(E):
                z.writestr(f"{run_id}/{e}/", b"")
                z.writestr(f"{run_id}/{e}/Images/", b"")
            for e, c, k, data in blobs:
                z.writestr(f"{run_id}/{e}/Images/cam{c}_image{30 + k}.png", data)
        del blobs
        src = host.Run(kind="zip", run_folder=os.path.join(tmp, "png", run_id))
        pdir = os.path.join(tmp, "packed", run_id)
        rp = src.repack(pdir, nthreads=16, ncams=C)
        src.close()
        os.makedirs(os.path.join(tmp, "pzip"))
        zpk = os.path.join(tmp, "pzip", run_id + ".zip")
        zip_dir(pdir, zpk)
        sources = {"png_zip": ("zip", os.path.join(tmp, "png", run_id)), "packed_dir": ("raw", pdir + "/"),
                   "packed_zip": ("zip", os.path.join(tmp, "pzip", run_id))}
        runs, texts = {}, {}
        for tag, (kind, where) in sources.items():
            runs[tag] = host.Run(kind=kind, run_folder=where)
            assert all(runs[tag].train(c, shape=(H, W))[0] == 0 for c in range(C))
        res = {tag: [] for tag in sources}
        if parent:
            res["png_zip_parent_build"], res["png_zip_this_tree_own_process"] = [], []
        os.makedirs(os.path.join(tmp, "out"))
        for rep in range(3):
            # the parent commit's PNG path on the same archive, in a process of its own; then this tree's the same way
            for tag, tree in (("png_zip_parent_build", parent), ("png_zip_this_tree_own_process", ROOT)) if parent else ():
                pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--png-run", sources["png_zip"][1], "--trace-shape",
                                     f"{W}x{H}x{C}", "--frames", str(E * C * F)], env=dict(os.environ, ABUB_BENCH_TREE=os.path.abspath(tree)),
                                    capture_output=True, text=True, timeout=300)
                assert pr.returncode == 0, pr.stdout[-1000:] + pr.stderr[-1000:]
                res[tag].append(json.loads([l for l in pr.stdout.splitlines() if l.startswith("{")][-1]))
            for tag in sources:
                t0 = time.perf_counter()
                st = runs[tag].run_batched(C, os.path.join(tmp, "out") + "/", tag, 30)
                dt = time.perf_counter() - t0
                res[tag].append({"s": dt, "frames_per_s": E * C * F / dt, "decode_s": st["decode_s"], "gpu_s": st["gpu_s"],
                                 "gpudecode_s": st["gpudecode_s"], "batches": int(st["batches"]),
                                 "frames_gpu_decoded": int(st["frames_gpu_decoded"]), "frames_gpu_unpacked": int(st["frames_gpu_unpacked"])})
                texts[tag] = open(os.path.join(tmp, "out", f"abub3hs_{tag}.txt")).read().replace(tag, "RUN")
        for r in runs.values():
            r.close()
        tr = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-run", pdir + "/", "--trace-shape", f"{W}x{H}x{C}"],
                            env=dict(os.environ, ABUB_INGEST_TRACE="1"), capture_output=True, text=True, timeout=300)
        out = {"events": E, "frames": E * C * F, "repack": dict(rp, frames_per_s=(rp["packed"] + rp["copied"]) / rp["seconds"]),
               "same_text": texts["png_zip"] == texts["packed_dir"] == texts["packed_zip"], "runs": res,
               "median_frames_per_s": {t: statistics.median(r["frames_per_s"] for r in res[t]) for t in res},
               "packed_dir_worker_timeline": [l for l in tr.stderr.splitlines() if l.startswith(("batch", "worker"))]}
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def trace_run(where, shape):
    from autobub3hs_amd import host

    W, H, C = (int(x) for x in shape.split("x"))
    run = host.Run(kind="raw", run_folder=where)
    assert all(run.train(c, shape=(H, W))[0] == 0 for c in range(C))
    tmp = tempfile.mkdtemp(prefix="abub_abf_trace_")
    try:
        run.run_batched(C, tmp + "/", "t", 30)
    finally:
        run.close()
        shutil.rmtree(tmp, ignore_errors=True)


def bench_once(tree, dump):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", dump], cwd=tree,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def part_c(parent):
    tmp = tempfile.mkdtemp(prefix="abub_abf_ab_")
    try:
        series = {"parent": [], "tree": []}
        same = True
        for rep in range(3):
            dumps = {}
            for who, tree in (("parent", parent), ("tree", ROOT)):
                dumps[who] = os.path.join(tmp, f"{who}{rep}")
                res = bench_once(tree, dumps[who])
                series[who].append({"value": res["value"], "ms_per_step": res.get("ms_per_step")})
            names = sorted(os.listdir(dumps["parent"]))
            same = same and names == sorted(os.listdir(dumps["tree"])) and len(names) > 0 and \
                all(filecmp.cmp(os.path.join(dumps["parent"], f), os.path.join(dumps["tree"], f), shallow=False) for f in names)
        med = {k: statistics.median(r["value"] for r in v) for k, v in series.items()}
        return {"command": "bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR", "first_of_each_pair": "parent", "runs": series,
                "median_frames_per_s": med, "tree_over_parent": med["tree"] / med["parent"], "dumped_outputs_identical": same}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "abf.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--events", type=int, default=96)
    ap.add_argument("--trace-run", default=None)
    ap.add_argument("--png-run", default=None)
    ap.add_argument("--trace-shape", default="1280x1024x2")
    a = ap.parse_args()
    if a.trace_run:
        trace_run(a.trace_run, a.trace_shape)
        sys.exit(0)
    if a.png_run:
        png_run(a.png_run, a.trace_shape, a.frames)
        sys.exit(0)
    result = {}
    for part, fn in (("a", lambda: part_a(a.frames)), ("b", lambda: part_b(a.events, a.parent)), ("c", lambda: part_c(a.parent))):
        key = {"a": "kernel", "b": "end_to_end", "c": "parent_comparison"}[part]
        if part not in a.parts or (part == "c" and not a.parent):
            result[key] = "not measured"
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
