#!/usr/bin/env python3
"""BMP frames on the GPU ("BMP frames on the GPU") measured on one GPU box, in one call -> profiles/r13/bmp.json.
  (a) kernel: abub_bmp_decode_dev over 1024 resident 8-bit BMP frames (bottom-up, the full grey palette, as Pillow writes
      them) without a table and with a non-identity table, abub_abf_decode_dev over the packed form of the same frames and
      a device-to-device hipMemcpyAsync of 1024 * W * H bytes: five alternating launches each after a warm-up, device
      events, medians; at 1280x1024 and at 1680x1050;
  (b) end to end: a run of tools/ingest_bench.py's geometry written as BMP into a directory, with as many events as keep
      it at or below the bytes of that tool's 96-event PNG archive; RunBatched with ABUB_GPU_BMP=1 and =0, three
      alternating repetitions; the recon texts compared; the medians, the spread of each setting's repetitions and
      whether the two series overlap decide the default of ABUB_GPU_BMP;
  (c) parent comparison: bench.py --steps 20 --warmup 5, a built checkout of the parent commit (--parent DIR) and this
      tree, twelve runs in the balanced order T P P T T P P T T P P T (tools/verify_bench.py part_c_balanced).
usage: python3 tools/bmp_bench.py [--parts abc] [--parent DIR] [--out profiles/r13/bmp.json] [--frames 1024] [--events 96]"""
import argparse, io, json, os, shutil, statistics, sys, tempfile, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

READ_CEILING_TBPS, FILL_CEILING_TBPS = 6.14, 5.95  # DESIGN section 6 (profiles/r03/copy_ceiling.jsonl)


def bmp_bytes(img):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(img).save(b, format="BMP")
    return b.getvalue()


def part_a(n, W, H):
    import torch
    from autobub3hs_amd import hip, host, synth, _lib

    F = 41
    spec = synth.random_spec(W, H, F, 3, 0)
    fr = np.asarray(synth.render_event(W, H, spec, 3, 0))
    P = W * H
    bmp = [bmp_bytes(fr[k]) for k in range(F)]
    abf = [host.abf_encode(fr[k]) for k in range(F)]
    info = hip.bmp_parse(bmp[0], W, H)
    assert info["bpp"] == 8 and info["identity"] and not info["top_down"] and info["data_off"] == 1078
    dev = torch.device("cuda:0")

    def blob_of(files):
        blob, at = bytearray(), []
        for i in range(n):
            at.append((len(blob), len(files[i % F])))
            blob += files[i % F]
            blob += b"\0" * (-len(blob) % 16)
        return torch.frombuffer(blob, dtype=torch.uint8).to(dev), at

    b_files, b_at = blob_of(bmp)
    a_files, a_at = blob_of(abf)
    rec = np.zeros((n, 8), np.uint32)
    rec[:, 0], rec[:, 1] = [o for o, _ in b_at], [l for _, l in b_at]
    rec[:, 2], rec[:, 3], rec[:, 4] = info["data_off"], info["stride"], 8
    rec[:, 5] = 0xFFFFFFFF
    dst = np.arange(n, dtype=np.uint64) * P
    rec[:, 6], rec[:, 7] = dst & 0xFFFFFFFF, dst >> 32
    b_desc = torch.from_numpy(rec.view(np.int32).copy()).to(dev)
    rec[:, 5] = 0
    b_desc_lut = torch.from_numpy(rec.view(np.int32).copy()).to(dev)
    table = (255 - np.arange(256)).astype(np.uint8)
    b_luts = torch.from_numpy(table.copy()).to(dev)
    arec = np.zeros((n, 4), np.uint32)
    arec[:, 0], arec[:, 1] = [o for o, _ in a_at], [l for _, l in a_at]
    arec[:, 2], arec[:, 3] = dst & 0xFFFFFFFF, dst >> 32
    a_desc = torch.from_numpy(arec.view(np.int32).copy()).to(dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    out = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    other = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def go_bmp():
        _lib.check(L.abub_bmp_decode_dev(b_files.data_ptr(), b_files.numel(), b_desc.data_ptr(), n, None, 0, W, H, out.data_ptr(),
                                         out.numel(), status.data_ptr(), stream), "bmp")

    def go_bmp_lut():
        _lib.check(L.abub_bmp_decode_dev(b_files.data_ptr(), b_files.numel(), b_desc_lut.data_ptr(), n, b_luts.data_ptr(), 1, W, H,
                                         out.data_ptr(), out.numel(), status.data_ptr(), stream), "bmp")

    def go_abf():
        _lib.check(L.abub_abf_decode_dev(a_files.data_ptr(), a_files.numel(), a_desc.data_ptr(), n, W, H, out.data_ptr(),
                                         out.numel(), status.data_ptr(), stream), "abf")

    def go_copy():
        other.copy_(out, non_blocking=True)  # (one hipMemcpyAsync, device to device, of n * W * H bytes)

    def check(table=None):
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all()
        for k in range(0, n, max(1, n // 7)):
            want = fr[k % F] if table is None else table[fr[k % F]]
            assert np.array_equal(out[k].cpu().numpy(), want), k
        out.zero_()

    go_bmp()
    check()
    go_bmp_lut()
    check(table)
    go_abf()
    check()
    go_copy()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    runs = {"bmp": go_bmp, "bmp_table": go_bmp_lut, "abf": go_abf, "copy": go_copy}
    ms = {k: [] for k in runs}
    for _ in range(5):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    file_bytes = sum(l for _, l in b_at)
    floor_ms = (file_bytes / READ_CEILING_TBPS + n * P / FILL_CEILING_TBPS) / 1e9
    res = {"frames": n, "W": W, "H": H, "bmp_file_bytes": len(bmp[0]), "packed_MB_per_frame": sum(l for _, l in a_at) / n / 1e6,
           "ms": ms, "ms_median": med, "frames_per_s": {k: n / v * 1e3 for k, v in med.items()},
           "floor_ms_one_read_one_write": floor_ms, "measured_copy_ms": med["copy"],
           "bmp_times_above_floor": med["bmp"] / floor_ms, "bmp_table_times_above_floor": med["bmp_table"] / floor_ms,
           "bmp_over_measured_copy": med["bmp"] / med["copy"], "bmp_TBps_read_plus_written": (file_bytes + n * P) / med["bmp"] / 1e9,
           "bound": "not measured"}
    del b_files, a_files, out, other
    torch.cuda.empty_cache()
    return res


def part_b(E_png, W=1280, H=1024, F=41, C=2):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from autobub3hs_amd import host, synth

    run_id = "20200925_0"
    tmp = tempfile.mkdtemp(prefix="abub_bmp_")
    try:
        def stack(e, c):
            return synth.render_event(W, H, synth.random_spec(W, H, F, e, c, p_second=0.2), e, c)

        def png_size(job):  # the bytes of the frames in tools/ingest_bench.py's archive (level-1 PNG, stored)
            st, total = stack(*job), 0
            for k in range(F):
                b = io.BytesIO()
                Image.fromarray(st[k]).save(b, format="PNG", compress_level=1)
                total += len(b.getvalue())
            return total

        nthr = min(16, len(os.sched_getaffinity(0)))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(nthr) as ex:
            archive = sum(ex.map(png_size, [(e, c) for e in range(E_png) for c in range(C)]))
        per_event = C * F * (1078 + ((W + 3) & ~3) * H)
        E = max(1, min(E_png, archive // per_event))
        rd = os.path.join(tmp, run_id)

        def write(job):
            e, c = job
            st = stack(e, c)
            d = os.path.join(rd, str(e), "Images")
            os.makedirs(d, exist_ok=True)
            for k in range(F):
                Image.fromarray(st[k]).save(os.path.join(d, f"cam{c}_image{30 + k}.bmp"))

        with ThreadPoolExecutor(nthr) as ex:
            list(ex.map(write, [(e, c) for e in range(E) for c in range(C)]))
        with open(os.path.join(rd, run_id + ".txt"), "w") as f:
            for e in range(E):
                f.write(f"{run_id} {e} a b c d e f g h i\n")
        made_s = time.perf_counter() - t0
        run = host.Run("raw", rd + "/", "Images", "cam%d_image%u.bmp")
        assert all(run.train(c, shape=(H, W))[0] == 0 for c in range(C))
        res, texts = {"on": [], "off": []}, {}
        os.makedirs(os.path.join(tmp, "out"))
        for rep in range(3):
            for tag in ("on", "off"):
                os.environ["ABUB_GPU_BMP"] = "1" if tag == "on" else "0"
                t0 = time.perf_counter()
                st = run.run_batched(C, os.path.join(tmp, "out") + "/", tag, 30)
                dt = time.perf_counter() - t0
                res[tag].append({"s": dt, "frames_per_s": E * C * F / dt, "read_s": st["decode_s"], "upload_plus_decode_s": st["gpudecode_s"],
                                 "gpu_s": st["gpu_s"], "batches": int(st["batches"]), "frames_gpu_bmp": int(st["frames_gpu_bmp"]),
                                 "frames_gpu_decoded": int(st["frames_gpu_decoded"]), "frames_host_decoded": int(st["frames_host_decoded"])})
                texts[tag] = open(os.path.join(tmp, "out", f"abub3hs_{tag}.txt")).read().replace(tag, "RUN")
                print("bmp_bench:", tag, json.dumps(res[tag][-1]), flush=True)
        os.environ.pop("ABUB_GPU_BMP")
        run.close()
        med = {t: statistics.median(r["frames_per_s"] for r in res[t]) for t in res}
        spread = {t: max(r["frames_per_s"] for r in res[t]) - min(r["frames_per_s"] for r in res[t]) for t in res}
        return {"png_archive_events": E_png, "png_archive_frame_bytes": archive, "events": E, "frames": E * C * F,
                "bmp_run_bytes": E * per_event, "made_in_s": made_s, "same_text": texts["on"] == texts["off"], "runs": res,
                "median_frames_per_s": med, "spread_frames_per_s": spread,
                "off_minus_on_median_frames_per_s": med["off"] - med["on"],
                "every_off_run_above_every_on_run": min(r["frames_per_s"] for r in res["off"]) > max(r["frames_per_s"] for r in res["on"])}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "bmp.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--events", type=int, default=96)
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):  # (a part measured by an earlier call stays)
        result = json.load(open(a.out))

    def part_c():
        import verify_bench

        return verify_bench.part_c_balanced(a.parent, "TPPTTPPTTPPT")

    parts = (("a", "kernel", lambda: {"1280x1024": part_a(a.frames, 1280, 1024), "1680x1050": part_a(a.frames, 1680, 1050)}),
             ("b", "end_to_end", lambda: part_b(a.events)), ("c", "parent_comparison", part_c))
    for part, key, fn in parts:
        if part not in a.parts or (part == "c" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
