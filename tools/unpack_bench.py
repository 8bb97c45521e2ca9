#!/usr/bin/env python3
"""abub_png_encode_dev and abub3hs --unpack [--unpack-gpu] measured on one GPU box, in one call -> profiles/r12/unpack.json.
  (a) kernel: abub_png_encode_dev on 1024 resident 1280x1024 synth frames and, next to it, abub_abf_encode_dev on the same
      frames, alternating five times each after a warm-up, device events, medians; the floor of one read of the frames and
      one write of the files at the ceilings of DESIGN section 6, and how far above it the encoder is;
      --kernel-only: just the two encoders, three times each (the program of a `rocprofv3 --kernel-trace --stats` run);
  (b) sizes: bytes per frame of the canonical Huffman-only PNG against the ABF1 file, the level-1 PNG and zlib
      Z_HUFFMAN_ONLY over the same filtered bytes, for the synth frames and for the sample frame;
  (c) end to end: the 96-event archive of tools/ingest_bench.py (a stored PNG zip), repacked once; Run.unpack on 16 threads
      against Run.unpack(device=0) of the packed directory, three alternating repetitions, medians, the device route's legs;
  (d) decode rate: abub_png_decode_dev on the Huffman-only files against the level-1 files of the same frames, and RunBatched
      on the unpacked run against the level-1 PNG run, three alternating repetitions;
  (e) parent comparison: bench.py --steps 20 --warmup 5, the parent build and this tree in the balanced order
      T P P T T P P T T P P T (tools/verify_bench.py part_c_balanced), dumped outputs compared byte for byte.
usage: python3 tools/unpack_bench.py [--parts abcde] [--parent DIR] [--order ORDER] [--out profiles/r12/unpack.json] [--frames 1024]
       [--events 96] [--kernel-only]"""
import argparse, io, json, os, shutil, statistics, sys, tempfile, zipfile, zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

READ_CEILING_TBPS, FILL_CEILING_TBPS = 6.14, 5.95  # DESIGN section 6 (profiles/r03/copy_ceiling.jsonl)


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def synth_frames(W, H, F=41):
    from autobub3hs_amd import synth
    return np.asarray(synth.render_event(W, H, synth.random_spec(W, H, F, 3, 0), 3, 0))


def level1(img):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG", compress_level=1)
    return b.getvalue()


def huffman_only_zlib(img):
    """zlib with Z_HUFFMAN_ONLY over the Sub-filtered bytes, in the same container (63 bytes around the deflate data)"""
    f = np.empty((img.shape[0], img.shape[1] + 1), np.uint8)
    f[:, 0], f[:, 1], f[:, 2:] = 1, img[:, 0], img[:, 1:] - img[:, :-1]
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    return 8 + 25 + 12 + len(c.compress(f.tobytes()) + c.flush()) + 12


def encoders(n, W, H, fr):
    """-> (go_png, go_abf, read back) over n resident frames"""
    import torch
    from autobub3hs_amd import _lib
    L, dev, P, F = _lib.lib(), torch.device("cuda:0"), W * H, len(fr)
    frames = torch.from_numpy(fr).to(dev)[torch.arange(n, device=dev) % F].contiguous().reshape(-1)
    src = torch.arange(n, dtype=torch.int64, device=dev) * P
    stream = torch.cuda.current_stream().cuda_stream
    st = {}
    for tag, bound, scr, fn in (("png", L.abub_png_file_bound, L.abub_png_encode_scratch_bytes, L.abub_png_encode_dev),
                                ("abf", L.abub_abf_file_bound, L.abub_abf_encode_scratch_bytes, L.abub_abf_encode_dev)):
        cap = n * ((int(bound(W, H)) + 15) & ~15) if tag == "abf" else n * (P + 4096)  # (the PNG bound is 15 bits per symbol)
        st[tag] = dict(out=torch.empty(cap, dtype=torch.uint8, device=dev), files=torch.zeros((n, 2), dtype=torch.int64, device=dev),
                       total=torch.zeros(1, dtype=torch.int64, device=dev),
                       scratch=torch.empty(int(scr(n, W, H)), dtype=torch.uint8, device=dev), fn=fn)

    def go(tag):
        s = st[tag]
        _lib.check(s["fn"](frames.data_ptr(), frames.numel(), src.data_ptr(), n, W, H, s["out"].data_ptr(), s["out"].numel(),
                           s["files"].data_ptr(), s["total"].data_ptr(), s["scratch"].data_ptr(), s["scratch"].numel(), stream), tag)

    def back(tag, k):
        rec = st[tag]["files"].cpu().numpy()
        assert ((rec[:, 1] >> 32) == 0).all(), "a file did not fit"
        o, l = int(rec[k, 0]), int(rec[k, 1] & 0xFFFFFFFF)
        return st[tag]["out"][o:o + l].cpu().numpy().tobytes(), int(st[tag]["total"].item())

    return (lambda: go("png")), (lambda: go("abf")), back


def part_a(n, W=1280, H=1024, kernel_only=False):
    import torch
    from autobub3hs_amd import host
    fr = synth_frames(W, H)
    go_png, go_abf, back = encoders(n, W, H, fr)
    go_png()
    go_abf()
    torch.cuda.synchronize()
    if kernel_only:
        for _ in range(3):
            go_png()
            go_abf()
        torch.cuda.synchronize()
        return None
    for k in (0, n // 3, n - 1):
        assert back("png", k)[0] == host.png_huff_encode(fr[k % len(fr)]), k
        assert back("abf", k)[0] == host.abf_encode(fr[k % len(fr)]), k
    t_png, t_abf = [], []
    for _ in range(5):
        t_png.append(timed(go_png))
        t_abf.append(timed(go_abf))
    P, png_bytes, abf_bytes = W * H, back("png", 0)[1], back("abf", 0)[1]
    ms, ms_abf = statistics.median(t_png), statistics.median(t_abf)
    floor = (n * P / READ_CEILING_TBPS + png_bytes / FILL_CEILING_TBPS) / 1e9
    return {"frames": n, "W": W, "H": H, "png_encode_ms": t_png, "abf_encode_ms": t_abf, "png_encode_ms_median": ms,
            "abf_encode_ms_median": ms_abf, "png_frames_per_s": n / ms * 1e3, "abf_frames_per_s": n / ms_abf * 1e3,
            "png_over_abf": ms / ms_abf, "png_file_bytes": png_bytes, "abf_file_bytes": abf_bytes,
            "floor_ms_one_read_one_write": floor, "times_above_floor": ms / floor,
            "pixels_read_TBps_at_three_reads": 3 * n * P / ms / 1e9}


def part_b(W=1280, H=1024):
    from PIL import Image
    from autobub3hs_amd import host
    fr = synth_frames(W, H)
    sample = np.array(Image.open(os.path.join(ROOT, "tests", "golden", "sample_40l19_cam1_image30.png")).convert("L"))

    def sizes(imgs):
        rows = [(len(host.png_huff_encode(im)), len(host.abf_encode(im)), len(level1(im)), huffman_only_zlib(im)) for im in imgs]
        m = np.mean(np.array(rows, float), axis=0)
        return {"frames": len(imgs), "huffman_only_png": m[0], "abf1": m[1], "png_level_1": m[2], "zlib_Z_HUFFMAN_ONLY_same_filter": m[3],
                "over_abf1": m[0] / m[1], "over_png_level_1": m[0] / m[2], "over_zlib_huffman_only": m[0] / m[3]}

    return {"synth_1280x1024_bytes_per_frame": sizes(list(fr)), "sample_frame_1680x1050_bytes": sizes([sample])}


def png_decoder(files, n, W, H):
    """abub_png_decode_dev over n frames taken round robin from `files` -> (go, check)"""
    import torch
    from autobub3hs_amd import hip, _lib
    dev, P, F = torch.device("cuda:0"), W * H, len(files)
    frames_np = np.zeros((n, 8), dtype=np.uint32)
    segs, blob, zoff = [], bytearray(), 0
    for i in range(n):
        data = files[i % F]
        sg, lut = hip.png_parse(data, W, H)
        base, zlen = len(blob), sum(l for _, l in sg)
        frames_np[i] = (len(segs), len(sg), zoff, zlen, 0xFFFFFFFF, 0, (i * P) & 0xFFFFFFFF, (i * P) >> 32)
        segs += [(base + o, l) for o, l in sg]
        blob += data
        blob += b"\0" * ((-len(blob)) % 4)
        zoff += ((zlen + 15) & ~15) + 16
    blob += b"\0" * 8
    t = dict(files=torch.frombuffer(blob, dtype=torch.uint8).to(dev), frames=torch.from_numpy(frames_np.view(np.int32).copy()).to(dev),
             segs=torch.tensor(segs, dtype=torch.int64).to(torch.int32).to(dev), luts=torch.zeros(256, dtype=torch.uint8, device=dev),
             z=torch.empty((zoff,), dtype=torch.uint8, device=dev),
             raw=torch.empty((n * int(_lib.lib().abub_png_raw_stride(W, H)),), dtype=torch.uint8, device=dev),
             status=torch.zeros(n, dtype=torch.int32, device=dev), out=torch.zeros((n, H, W), dtype=torch.uint8, device=dev))
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream

    def go():
        _lib.check(L.abub_png_decode_dev(t["files"].data_ptr(), t["files"].numel(), t["frames"].data_ptr(), n, t["segs"].data_ptr(),
                                         len(segs), t["luts"].data_ptr(), 0, W, H, t["z"].data_ptr(), t["z"].numel(), t["raw"].data_ptr(),
                                         t["raw"].numel(), t["out"].data_ptr(), t["out"].numel(), t["status"].data_ptr(), stream), "png")

    def check(fr):
        torch.cuda.synchronize()
        assert (t["status"].cpu().numpy() == 0).all(), "the GPU decoder refused a file"
        for k in range(0, n, max(1, n // 5)):
            assert np.array_equal(t["out"][k].cpu().numpy(), fr[k % F]), k

    return go, check


def part_d_kernel(n, W=1280, H=1024):
    import torch
    from autobub3hs_amd import host
    fr = synth_frames(W, H)
    res = {}
    for tag, files in (("huffman_only", [host.png_huff_encode(im) for im in fr]), ("level_1", [level1(im) for im in fr])):
        go, check = png_decoder(files, n, W, H)
        go()
        check(fr)
        res[tag] = {"ms": [timed(go) for _ in range(5)], "MB_per_frame": sum(map(len, files)) / len(files) / 1e6}
        del go, check
        torch.cuda.empty_cache()
    for tag in res:
        res[tag]["ms_median"] = statistics.median(res[tag]["ms"])
        res[tag]["frames_per_s"] = n / res[tag]["ms_median"] * 1e3
    return {"frames": n, "W": W, "H": H, "abub_png_decode_dev": res,
            "huffman_only_over_level_1_time": res["huffman_only"]["ms_median"] / res["level_1"]["ms_median"]}


def part_cd(E, parts, W=1280, H=1024, F=41, C=2):
    from concurrent.futures import ThreadPoolExecutor
    from autobub3hs_amd import host, synth

    run_id = "20200925_0"
    tmp = tempfile.mkdtemp(prefix="abub_unpack_")
    out = {}
    try:
        def enc(job):
            e, c = job
            st = synth.render_event(W, H, synth.random_spec(W, H, F, e, c, p_second=0.2), e, c)
            return [(e, c, k, level1(st[k])) for k in range(F)]

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
        print("unpack_bench: archive written", flush=True)
        total = E * C * F
        src = host.Run(kind="zip", run_folder=os.path.join(tmp, "png", run_id))
        packed = os.path.join(tmp, "packed", run_id)
        st = src.repack(packed, nthreads=16, ncams=C, device=0)
        assert st["packed"] == total and st["failed"] == 0
        print("unpack_bench: repacked", flush=True)
        prun = host.Run(kind="raw", run_folder=packed + "/")
        res = {"host": [], "gpu": []}
        dirs = {}
        for rep in range(3):
            for tag, device in (("host", None), ("gpu", 0)):
                dirs[tag] = os.path.join(tmp, f"unpacked_{tag}", run_id)
                shutil.rmtree(os.path.dirname(dirs[tag]), ignore_errors=True)
                r = prun.unpack(dirs[tag], nthreads=16, ncams=C, device=device)
                assert r["packed"] == total and r["failed"] == 0 and r["copied"] == 0, r
                assert device is None or (r["device"] == 0 and r["frames_gpu_encoded"] == total), r
                res[tag].append(dict(r, frames_per_s=total / r["seconds"]))
                print(f"unpack_bench: unpack {tag} {rep}: {res[tag][-1]['frames_per_s']:.0f} frames/s", flush=True)
        a = open(os.path.join(dirs["host"], "7", "Images", "cam1_image50.png"), "rb").read()
        assert a == open(os.path.join(dirs["gpu"], "7", "Images", "cam1_image50.png"), "rb").read() and a[:4] == b"\x89PNG"
        urun = host.Run(kind="raw", run_folder=dirs["gpu"] + "/")
        v = src.verify(urun, nthreads=16, ncams=C, device=0)
        assert v["rc"] == 0 and v["same_not_packed"] == total, {k: x for k, x in v.items() if k != "findings"}
        med = {t: statistics.median(r["frames_per_s"] for r in res[t]) for t in res}
        legs = ("read_s", "decode_s", "encode_s", "copy_s", "write_s", "seconds")
        out["end_to_end"] = {"events": E, "frames": total, "source": "directory of packed frames", "runs": res,
                             "median_frames_per_s": med, "gpu_over_host": med["gpu"] / med["host"],
                             "gpu_route_legs_s_median": {k: statistics.median(r[k] for r in res["gpu"]) for k in legs},
                             "gpu_route_batches": int(res["gpu"][0]["batches"]), "bytes_out": res["gpu"][0]["bytes_out"],
                             "verify_gpu_of_the_unpacked_run": "every frame same_not_packed"}
        if "d" in parts:
            rb = {"unpacked": [], "level_1_zip": []}
            texts = {}
            for run in (urun, src):
                assert all(run.train(c, shape=(H, W))[0] == 0 for c in range(C))
            for rep in range(3):
                for tag, run in (("unpacked", urun), ("level_1_zip", src)):
                    o = tempfile.mkdtemp(prefix="abub_unpack_out_", dir=tmp)
                    s = run.run_batched(C, o + "/", "t", 30)
                    texts[tag] = open(os.path.join(o, "abub3hs_t.txt"), "rb").read()
                    rb[tag].append(dict(s, frames_per_s=s["frames"] / s["total_s"]))
                    print(f"unpack_bench: RunBatched {tag} {rep}: {rb[tag][-1]['frames_per_s']:.0f} frames/s", flush=True)
            medb = {t: statistics.median(r["frames_per_s"] for r in rb[t]) for t in rb}
            out["run_batched"] = {"runs": rb, "median_frames_per_s": medb, "unpacked_over_level_1": medb["unpacked"] / medb["level_1_zip"],
                                  "same_text": texts["unpacked"] == texts["level_1_zip"],
                                  "frames_gpu_decoded_unpacked_run": rb["unpacked"][0]["frames_gpu_decoded"]}
        for run in (src, prun, urun):
            run.close()
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abcde")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--order", default="TPPTTPPTTPPT")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "unpack.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--events", type=int, default=96)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    if a.kernel_only:
        part_a(a.frames, kernel_only=True)
        sys.exit(0)
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}  # (a second call adds to the first)

    def save(key, value):
        result[key] = value
        print(json.dumps({key: value}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)

    if "a" in a.parts:
        save("kernel", part_a(a.frames))
    if "b" in a.parts:
        save("sizes", part_b())
    if "d" in a.parts:
        save("decode_kernel", part_d_kernel(a.frames))
    if "c" in a.parts:
        for k, v in part_cd(a.events, a.parts).items():
            save(k, v)
    if "e" in a.parts and a.parent:
        import verify_bench
        save("parent_comparison_" + a.order, verify_bench.part_c_balanced(a.parent, a.order))
