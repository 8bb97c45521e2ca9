#!/usr/bin/env python3
"""Deflated zip entries inflated on the GPU ("Deflated zip entries on the GPU") measured on one GPU box, in
one call -> profiles/r14/unzip.json.
  (a) kernel: abub_unzip_dev (inflate + CRC-32) over 1024 resident entries of 1280x1024 synth frames, stored as level-1 PNG
      files and deflated again by the zip layer (level 6, what zip tools do), and the same frames stored as 8-bit BMP files
      and deflated; abub_crc32_dev alone over the inflated files; five alternating launches each after a warm-up, device
      events, medians; beside them the host's inflate of the same entries (zlib, raw streams) on 16 threads;
  (b) end to end: a deflated archive of each kind, --events events as tools/ingest_bench.py, RunBatched with ABUB_GPU_UNZIP
      unset and =1, three alternating repetitions, medians, the recon texts compared; the BMP archive with ABUB_GPU_BMP=1 and
      once more with it unset (the BMP decoder off: the whole run takes the host route and the knob has no effect);
  (c) parent comparison: bench.py --steps 20 --warmup 5, a built checkout of the parent commit (--parent DIR) and this
      tree, twelve runs in the balanced order T P P T T P P T T P P T (tools/verify_bench.py part_c_balanced).
usage: python3 tools/unzip_bench.py [--parts abc] [--parent DIR] [--out profiles/r14/unzip.json] [--entries 1024] [--events 96]"""
import argparse, io, json, os, shutil, statistics, struct, sys, tempfile, time, zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

W, H, F, C = 1280, 1024, 41, 2


def png_bytes(img):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="PNG", compress_level=1)
    return b.getvalue()


def bmp_bytes(img):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, format="BMP")
    return b.getvalue()


def deflate_raw(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def align16(n):
    return (n + 15) & ~15


def part_a(n):
    import torch
    from autobub3hs_amd import synth, _lib

    fr = np.asarray(synth.render_event(W, H, synth.random_spec(W, H, F, 3, 0), 3, 0))
    dev = torch.device("cuda:0")
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    kinds = {}
    for kind, enc in (("png", png_bytes), ("bmp", bmp_bytes)):
        files = [enc(fr[k]) for k in range(F)]
        zs = [deflate_raw(f) for f in files]
        comp, rec, dst = bytearray(), np.zeros((n, 6), np.uint32), 0
        for i in range(n):
            z, f = zs[i % F], files[i % F]
            rec[i] = (len(comp), len(z), len(f), zlib.crc32(f) & 0xFFFFFFFF, dst & 0xFFFFFFFF, dst >> 32)
            comp += z + bytes(align16(len(z)) - len(z) + 16)
            dst += align16(len(f))
        kinds[kind] = dict(files=files, zs=zs, comp=torch.frombuffer(comp, dtype=torch.uint8).to(dev), out_bytes=dst,
                           ent=torch.from_numpy(rec.view(np.int32).copy()).to(dev), rec=rec)
    out = torch.zeros(max(k["out_bytes"] for k in kinds.values()), dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    crc = torch.zeros(n, dtype=torch.int32, device=dev)

    def unzip(kind):
        k = kinds[kind]
        _lib.check(L.abub_unzip_dev(k["comp"].data_ptr(), k["comp"].numel(), k["ent"].data_ptr(), n, out.data_ptr(), k["out_bytes"],
                                    status.data_ptr(), stream), "abub_unzip_dev")

    def crc_only(kind):
        k = kinds[kind]
        _lib.check(L.abub_crc32_dev(out.data_ptr(), k["out_bytes"], k["ent"].data_ptr(), n, crc.data_ptr(), status.data_ptr(), stream),
                   "abub_crc32_dev")

    for kind, k in kinds.items():  # warm-up and check
        unzip(kind)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all(), kind
        for i in range(0, n, max(1, n // 7)):
            o = int(k["rec"][i, 4]) | (int(k["rec"][i, 5]) << 32)
            assert out[o:o + len(k["files"][i % F])].cpu().numpy().tobytes() == k["files"][i % F], (kind, i)
        crc_only(kind)
        torch.cuda.synchronize()
        assert ((crc.cpu().numpy().astype(np.int64) & 0xFFFFFFFF) == k["rec"][:, 3]).all(), kind

    def timed(fn, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*args)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms = {"unzip_png": [], "unzip_bmp": [], "crc_png": [], "crc_bmp": []}
    for _ in range(5):
        for kind in ("png", "bmp"):
            ms["unzip_" + kind].append(timed(unzip, kind))
            ms["crc_" + kind].append(timed(crc_only, kind))  # (over what the launch before has just inflated)
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"entries": n, "W": W, "H": H, "ms": ms, "ms_median": med, "entries_per_s": {k: n / v * 1e3 for k, v in med.items()}}
    nthr = min(16, len(os.sched_getaffinity(0)))
    for kind, k in kinds.items():
        zs = [k["zs"][i % F] for i in range(n)]
        with ThreadPoolExecutor(nthr) as ex:
            t0 = time.perf_counter()
            sizes = list(ex.map(lambda z: len(zlib.decompress(z, -15)), zs))
            dt = time.perf_counter() - t0
        assert sizes == [len(k["files"][i % F]) for i in range(n)]
        res["host_" + kind] = {"threads": nthr, "s": dt, "entries_per_s": n / dt, "ms_per_entry_and_core": dt * nthr / n * 1e3}
        res["compressed_MB_per_entry_" + kind] = sum(len(z) for z in k["zs"]) / F / 1e6
        res["file_MB_per_entry_" + kind] = sum(len(f) for f in k["files"]) / F / 1e6
        res["gpu_over_host_" + kind] = res["entries_per_s"]["unzip_" + kind] / res["host_" + kind]["entries_per_s"]
    del out, kinds
    torch.cuda.empty_cache()
    return res


def write_zip(path, entries, big=0xFFFFFFFF):
    """entries: (name, crc, ulen, method, stream); zip64 records where an offset or the directory needs them (big: from which
    offset on, for a check of those records on a small archive)"""
    cd, n = bytearray(), 0
    with open(path, "wb") as f:
        for name, crc, ulen, method, stream in entries:
            nm, off = name.encode(), f.tell()
            f.write(struct.pack("<IHHHHHIIIHH", 0x04034B50, 20, 0, method, 0, 0x21, crc, len(stream), ulen, len(nm), 0) + nm)
            f.write(stream)
            extra = struct.pack("<HHQ", 1, 8, off) if off >= big else b""
            cd += struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 45, 45 if extra else 20, 0, method, 0, 0x21, crc, len(stream), ulen, len(nm),
                              len(extra), 0, 0, 0, 0x10 if name.endswith("/") else 0, 0xFFFFFFFF if extra else off) + nm + extra
            n += 1
        cdoff = f.tell()
        f.write(cd)
        f.write(struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, n, n, len(cd), cdoff))
        f.write(struct.pack("<IIQI", 0x07064B50, 0, cdoff + len(cd), 1))
        f.write(struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, min(n, 0xFFFF), min(n, 0xFFFF), min(len(cd), 0xFFFFFFFF), 0xFFFFFFFF if cdoff >= big else cdoff, 0))


def part_b(E_png):
    from autobub3hs_amd import host, synth

    run_id = "20200925_0"
    tmp = tempfile.mkdtemp(prefix="abub_unzip_")
    nthr = min(16, len(os.sched_getaffinity(0)))
    result = {}
    try:
        for kind, enc, E, envs in (("png", png_bytes, E_png, ({},)), ("bmp", bmp_bytes, E_png, ({"ABUB_GPU_BMP": "1"}, {}))):
            t0 = time.perf_counter()

            def make(job):
                e, c = job
                st = synth.render_event(W, H, synth.random_spec(W, H, F, e, c, p_second=0.2), e, c)
                out = []
                for k in range(F):
                    data = enc(st[k])
                    out.append((f"{run_id}/{e}/Images/cam{c}_image{30 + k}.png", zlib.crc32(data) & 0xFFFFFFFF, len(data), 8, deflate_raw(data)))
                return out

            entries = [(run_id + "/", 0, 0, 0, b"")]
            for e in range(E):
                entries += [(f"{run_id}/{e}/", 0, 0, 0, b""), (f"{run_id}/{e}/Images/", 0, 0, 0, b"")]
            with ThreadPoolExecutor(nthr) as ex:
                for l in ex.map(make, [(e, c) for e in range(E) for c in range(C)]):
                    entries += l
            files_bytes, comp_bytes = sum(x[2] for x in entries), sum(len(x[4]) for x in entries)
            d = os.path.join(tmp, kind)
            os.makedirs(os.path.join(d, "out"))
            write_zip(os.path.join(d, run_id + ".zip"), entries)
            del entries
            made_s = time.perf_counter() - t0
            run = host.Run("zip", os.path.join(d, run_id), "Images", "cam%d_image%u.png")
            assert all(run.train(c, shape=(H, W))[0] == 0 for c in range(C))
            for env in envs:  # (the BMP archive twice: the BMP decoder on, and unset -- the host route, where the knob has no effect)
                key = kind if env or kind == "png" else kind + "_decoder_unset"
                for k, v in env.items():
                    os.environ[k] = v
                res, texts = {"off": [], "on": []}, {}
                for rep in range(3):
                    for tag in ("off", "on"):
                        os.environ.pop("ABUB_GPU_UNZIP", None)
                        if tag == "on":
                            os.environ["ABUB_GPU_UNZIP"] = "1"
                        t0 = time.perf_counter()
                        st = run.run_batched(C, os.path.join(d, "out") + "/", tag, 30)
                        dt = time.perf_counter() - t0
                        res[tag].append({"s": dt, "frames_per_s": E * C * F / dt, "read_s": st["decode_s"], "unzip_device_s": st["unzip_s"],
                                         "upload_plus_decode_s": st["gpudecode_s"], "gpu_s": st["gpu_s"], "batches": int(st["batches"]),
                                         "frames_gpu_unzipped": int(st["frames_gpu_unzipped"]), "frames_gpu_decoded": int(st["frames_gpu_decoded"]),
                                         "frames_host_decoded": int(st["frames_host_decoded"])})
                        texts[tag] = open(os.path.join(d, "out", f"abub3hs_{tag}.txt")).read().replace(tag, "RUN")
                        print("unzip_bench:", key, tag, json.dumps(res[tag][-1]), flush=True)
                os.environ.pop("ABUB_GPU_UNZIP", None)
                for k in env:
                    os.environ.pop(k)
                med = {t: statistics.median(r["frames_per_s"] for r in res[t]) for t in res}
                result[key] = {"events": E, "frames": E * C * F, "file_bytes": files_bytes, "archive_stream_bytes": comp_bytes, "made_in_s": made_s,
                               "env": env, "same_text": texts["on"] == texts["off"], "runs": res, "median_frames_per_s": med,
                               "spread_frames_per_s": {t: max(r["frames_per_s"] for r in res[t]) - min(r["frames_per_s"] for r in res[t]) for t in res},
                               "on_over_off": med["on"] / med["off"],
                               "every_on_run_above_every_off_run": min(r["frames_per_s"] for r in res["on"]) > max(r["frames_per_s"] for r in res["off"])}
            run.close()
            shutil.rmtree(d, ignore_errors=True)
        return result
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "unzip.json"))
    ap.add_argument("--entries", type=int, default=1024)
    ap.add_argument("--events", type=int, default=96)
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):  # (a part measured by an earlier call stays)
        result = json.load(open(a.out))

    def part_c():
        import verify_bench

        return verify_bench.part_c_balanced(a.parent, "TPPTTPPTTPPT")

    parts = (("a", "kernel", lambda: part_a(a.entries)), ("b", "end_to_end", lambda: part_b(a.events)), ("c", "parent_comparison", part_c))
    for part, key, fn in parts:
        if part not in a.parts or (part == "c" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
