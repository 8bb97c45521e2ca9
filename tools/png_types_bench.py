#!/usr/bin/env python3
"""PNG types on the GPU ("PNG types on the GPU") measured on one GPU box -> profiles/r15/png_types.json.
  (a) kernel: 1024 resident 1280x1024 synth frames (fewer where 1024 files exceed the 4 GB a launch takes) written as RGB 8
      and grey 16 (Pillow, compress_level 1, its adaptive row filters) and RGBA 16 (tests/pngtypes.py, row by row the filter
      types Pillow chose for the RGB 8 file of the same image; random low bytes and alpha): abub_png_decode_typed_dev on
      each, next to abub_png_decode_dev on the 8-bit grey files of the same images, five alternating launches each after a
      warm-up, device events, medians; and 16 host threads decoding the same files (host.imdecode);
  (b) end to end: RunBatched on a directory of the RGB 8 run (tools/ingest_bench.py's geometry, --events events),
      ABUB_GPU_PNG_TYPES=1 against unset, three alternating repetitions, medians, the recon texts compared;
  (c) nothing else moved: tools/png_bench.py 1024 1 (the 8-bit decode) and bench.py --steps 20 --warmup 5, a built checkout of
      the parent commit (--parent DIR) and this tree alternating (--order, T: this tree, P: the parent).
usage: python3 tools/png_types_bench.py [--parts abc] [--parent DIR] [--out profiles/r15/png_types.json] [--frames 1024]
       [--events 24] [--order TPPTTP]"""
import argparse, io, json, os, re, shutil, statistics, subprocess, sys, tempfile, time, zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def pillow_png(arr, level=1):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(arr).save(b, format="PNG", compress_level=level)
    return b.getvalue()


def filter_types_of(png, W, H, row_bytes):
    """the filter type of every row of a PNG file"""
    from autobub3hs_amd import hip

    segs = hip.png_parse(png, W, H, types=True)[0]
    raw = zlib.decompress(b"".join(png[o:o + l] for o, l in segs))
    return list(raw[::row_bytes + 1][:H])


def files_of(fr):
    """-> {kind name: (files, expected frames)} for the frames fr [F, H, W]"""
    import pngtypes as pt

    rs = np.random.RandomState(15)
    F, H, W = fr.shape
    out = {"grey8": ([pillow_png(fr[k]) for k in range(F)], fr)}
    rgb = [pillow_png(np.repeat(fr[k][:, :, None], 3, axis=2)) for k in range(F)]
    out["rgb8"] = (rgb, fr)
    g16 = fr.astype(np.uint16) << 8 | rs.randint(0, 256, fr.shape).astype(np.uint16)
    out["grey16"] = ([pillow_png(g16[k]) for k in range(F)], fr)
    rgba = []
    for k in range(F):
        s = np.repeat((fr[k].astype(np.uint16) << 8)[:, :, None], 4, axis=2) | rs.randint(0, 256, (H, W, 4)).astype(np.uint16)
        rgba.append(pt.make_png(s, 6, 16, filter_types_of(rgb[k], W, H, 3 * W)))
    out["rgba16"] = (rgba, fr)
    return out


class Resident:
    """n files on the device with their descriptors: one launch per go()"""

    def __init__(self, files, W, H, typed):
        import torch
        from autobub3hs_amd import hip, _lib

        self.L, self.W, self.H, self.typed, self.n = _lib.lib(), W, H, typed, len(files)
        n, P = self.n, W * H
        rec = np.zeros((n, 8), dtype=np.uint32)
        segs, blob, zoff = [], bytearray(), 0
        self.stride = int(self.L.abub_png_raw_stride(W, H))
        for i, data in enumerate(files):
            sg, lut, kind = hip.png_parse(data, W, H, types=True)
            assert lut is None and (kind != 0) == typed
            self.stride = max(self.stride, int(self.L.abub_png_raw_stride_kind(W, H, kind)))
            zlen = sum(l for _, l in sg)
            rec[i] = (len(segs), len(sg), zoff, zlen, 0xFFFFFFFF, kind, (i * P) & 0xFFFFFFFF, (i * P) >> 32)
            segs += [(len(blob) + o, l) for o, l in sg]
            blob += data
            blob += b"\0" * ((-len(blob)) % 4)
            zoff += ((zlen + 15) & ~15) + 16
        blob += b"\0" * 8
        dev = torch.device("cuda:0")
        self.file_bytes = len(blob)
        self.files = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
        self.frames = torch.from_numpy(rec.view(np.int32).copy()).to(dev)
        self.segs = torch.tensor(segs, dtype=torch.int64).to(torch.int32).to(dev)
        self.nsegs = len(segs)
        self.luts = torch.zeros(256, dtype=torch.uint8, device=dev)
        self.z = torch.empty((zoff,), dtype=torch.uint8, device=dev)
        self.raw = torch.empty((n * self.stride,), dtype=torch.uint8, device=dev)
        self.out = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
        self.status = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.stream = torch.cuda.current_stream().cuda_stream

    def go(self):
        from autobub3hs_amd import _lib

        a = (self.files.data_ptr(), self.files.numel(), self.frames.data_ptr(), self.n, self.segs.data_ptr(), self.nsegs,
             self.luts.data_ptr(), 0, self.W, self.H, self.z.data_ptr(), self.z.numel(), self.raw.data_ptr(), self.raw.numel())
        b = (self.out.data_ptr(), self.out.numel(), self.status.data_ptr(), self.stream)
        if self.typed:
            _lib.check(self.L.abub_png_decode_typed_dev(*a, self.stride, *b), "abub_png_decode_typed_dev")
        else:
            _lib.check(self.L.abub_png_decode_dev(*a, *b), "abub_png_decode_dev")


def part_a(n, W=1280, H=1024):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from autobub3hs_amd import host, synth

    F = 41
    spec = synth.random_spec(W, H, F, 3, 0)
    fr = np.asarray(synth.render_event(W, H, spec, 3, 0))
    t0 = time.perf_counter()
    kinds = files_of(fr)
    made_s = time.perf_counter() - t0
    res = {"frames": n, "W": W, "H": H, "files_made_in_s": made_s, "kinds": {}}
    hist = {}
    for name, (files, want) in kinds.items():
        if name != "grey8":
            ft = np.bincount(filter_types_of(files[0], W, H, {"rgb8": 3, "grey16": 2, "rgba16": 8}[name] * W), minlength=5)
            hist[name] = [int(v) for v in ft]
    res["filter_types_of_frame_0"] = hist
    runs = {}
    count = {}
    for name, (files, want) in kinds.items():
        # (abub_png_seg.off is 32 bits: a launch takes less than 4 GB of files, which 1024 RGBA 16 files of this size are not)
        count[name] = min(n, int(3.6e9 // (max(len(f) for f in files) + 64)) // 64 * 64)
        r = Resident([files[i % F] for i in range(count[name])], W, H, name != "grey8")
        r.go()  # warm-up, and the check
        torch.cuda.synchronize()
        assert (r.status.cpu().numpy() == 0).all(), name
        for k in range(0, count[name], max(1, count[name] // 7)):
            assert np.array_equal(r.out[k].cpu().numpy(), want[k % F]), (name, k)
        r.out.zero_()
        runs[name] = r
    ms = {k: [] for k in runs}
    for _ in range(5):
        for k, r in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r.go()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    nthr = min(16, len(os.sched_getaffinity(0)))
    for name, (files, want) in kinds.items():
        nk = count[name]
        batch = [files[i % F] for i in range(nk)]
        with ThreadPoolExecutor(nthr) as ex:
            list(ex.map(host.imdecode, batch[:nthr]))
            t0 = time.perf_counter()
            got = list(ex.map(lambda d: host.imdecode(d, cap=W * H), batch))
            dt = time.perf_counter() - t0
        assert np.array_equal(got[5], want[5])
        med = statistics.median(ms[name])
        res["kinds"][name] = {"frames": nk, "MB_per_file": runs[name].file_bytes / nk / 1e6, "raw_stride_bytes": runs[name].stride,
                              "ms": ms[name], "ms_median": med, "gpu_frames_per_s": nk / med * 1e3, "host_threads": nthr,
                              "host_frames_per_s": nk / dt, "gpu_over_host": nk / med * 1e3 / (nk / dt)}
    g8 = res["kinds"]["grey8"]["gpu_frames_per_s"]
    for name in res["kinds"]:
        res["kinds"][name]["gpu_frames_per_s_over_grey8"] = res["kinds"][name]["gpu_frames_per_s"] / g8
    del runs
    torch.cuda.empty_cache()
    return res


def part_b(E, W=1280, H=1024, F=41, C=2):
    from concurrent.futures import ThreadPoolExecutor
    from autobub3hs_amd import host, synth

    run_id = "20200925_0"
    tmp = tempfile.mkdtemp(prefix="abub_pngtypes_")
    try:
        rd = os.path.join(tmp, run_id)

        def write(job):
            e, c = job
            st = synth.render_event(W, H, synth.random_spec(W, H, F, e, c, p_second=0.2), e, c)
            d = os.path.join(rd, str(e), "Images")
            os.makedirs(d, exist_ok=True)
            total = 0
            for k in range(F):
                data = pillow_png(np.repeat(st[k][:, :, None], 3, axis=2))
                total += len(data)
                open(os.path.join(d, f"cam{c}_image{30 + k}.png"), "wb").write(data)
            return total

        nthr = min(16, len(os.sched_getaffinity(0)))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(nthr) as ex:
            run_bytes = sum(ex.map(write, [(e, c) for e in range(E) for c in range(C)]))
        with open(os.path.join(rd, run_id + ".txt"), "w") as f:
            for e in range(E):
                f.write(f"{run_id} {e} a b c d e f g h i\n")
        made_s = time.perf_counter() - t0
        run = host.Run("raw", rd + "/", "Images")
        assert all(run.train(c, shape=(H, W))[0] == 0 for c in range(C))
        res, texts = {"on": [], "off": []}, {}
        os.makedirs(os.path.join(tmp, "out"))
        os.environ.pop("ABUB_GPU_DECODE", None)
        for rep in range(3):
            for tag in ("on", "off"):
                os.environ.pop("ABUB_GPU_PNG_TYPES", None)
                if tag == "on":
                    os.environ["ABUB_GPU_PNG_TYPES"] = "1"
                t0 = time.perf_counter()
                st = run.run_batched(C, os.path.join(tmp, "out") + "/", tag, 30)
                dt = time.perf_counter() - t0
                res[tag].append({"s": dt, "frames_per_s": E * C * F / dt, "total_s": st["total_s"], "list_s": st["list_s"], "write_s": st["write_s"],
                                 "read_s": st["decode_s"], "upload_plus_decode_s": st["gpudecode_s"],
                                 "gpu_s": st["gpu_s"], "batches": int(st["batches"]), "frames_gpu_decoded": int(st["frames_gpu_decoded"]),
                                 "frames_host_decoded": int(st["frames_host_decoded"]), "frames_failed": int(st["frames_failed"])})
                texts[tag] = open(os.path.join(tmp, "out", f"abub3hs_{tag}.txt")).read().replace(tag, "RUN")
                print("png_types_bench:", tag, json.dumps(res[tag][-1]), flush=True)
        os.environ.pop("ABUB_GPU_PNG_TYPES", None)
        run.close()
        med = {t: statistics.median(r["frames_per_s"] for r in res[t]) for t in res}
        return {"events": E, "frames": E * C * F, "run_bytes": run_bytes, "made_in_s": made_s, "same_text": texts["on"] == texts["off"],
                "runs": res, "median_frames_per_s": med, "on_over_off": med["on"] / med["off"],
                "every_on_run_above_every_off_run": min(r["frames_per_s"] for r in res["on"]) > max(r["frames_per_s"] for r in res["off"])}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def png_bench_once(tree):
    r = subprocess.run([sys.executable, os.path.join("tools", "png_bench.py"), "1024", "1"], cwd=tree, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return float(re.search(r"([\d.]+) ms per batch", r.stdout).group(1))


def part_c(parent, order):
    import verify_bench

    series = {"parent": [], "tree": []}
    for who in order:
        who = "tree" if who == "T" else "parent"
        series[who].append(png_bench_once(ROOT if who == "tree" else parent))
        print(f"png_types_bench: png_bench {who}: {series[who][-1]:.2f} ms", flush=True)
    med = {k: statistics.median(v) for k, v in series.items()}
    res = {"png_bench": {"command": "tools/png_bench.py 1024 1 (ms per batch, the best of three launches)", "order": " ".join(order),
                         "ms": series, "median_ms": med, "tree_over_parent_ms": med["tree"] / med["parent"]}}
    res["bench"] = verify_bench.part_c_balanced(parent, order)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "png_types.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--events", type=int, default=24)
    ap.add_argument("--order", default="TPPTTP")
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):  # (a part measured by an earlier call stays)
        result = json.load(open(a.out))
    parts = (("a", "kernel", lambda: part_a(a.frames)), ("b", "end_to_end", lambda: part_b(a.events)),
             ("c", "parent_comparison", lambda: part_c(os.path.abspath(a.parent), a.order)))
    for part, key, fn in parts:
        if part not in a.parts or (part == "c" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
