#!/usr/bin/env python3
"""The GPU encoder of the packed frame format and abub3hs --repack --repack-gpu measured on one GPU box, in one call ->
profiles/r10/repack.json.
  (a) kernel: abub_abf_encode_dev over 1024 resident 1280x1024 synth frames against abub_abf_decode_dev over the files it
      wrote, alternating five times each, device events, medians; the floor of one read of the frames and one write of the
      files at the ceilings of DESIGN section 6;
  (b) end to end: the 96-event archive of tools/ingest_bench.py (a stored PNG zip) through Run.repack (host route, 16
      threads) and Run.repack(device=0), three alternating repetitions, medians; the two trees compared file by file; the
      legs of the device route (read, upload + decode, encode, copy back, write) summed over its batches; the break-even
      count of re-analyses from the measured rates and the reading rates of DESIGN section 3 (10.8 k and 16.8 k frames/s);
  (c) parent comparison: tools/abf_bench.py part (c) (bench.py --steps 20 --warmup 5, parent build and this tree
      alternating, three runs each, dumped outputs compared byte for byte).
usage: python3 tools/repack_bench.py [--parts abc] [--parent DIR] [--out profiles/r10/repack.json] [--frames 1024] [--events 96]"""
import argparse, filecmp, io, json, os, shutil, statistics, sys, tempfile, zipfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

READ_CEILING_TBPS, FILL_CEILING_TBPS = 6.14, 5.95  # DESIGN section 6 (profiles/r03/copy_ceiling.jsonl)
PNG_READ_FPS, PACKED_READ_FPS = 10.8e3, 16.8e3     # DESIGN section 3, "Packed frames", (b)


def part_a(n, W=1280, H=1024):
    import torch
    from autobub3hs_amd import hip, host, synth, _lib

    F = 41
    spec = synth.random_spec(W, H, F, 3, 0)
    fr = np.asarray(synth.render_event(W, H, spec, 3, 0))
    P = W * H
    dev = torch.device("cuda:0")
    frames = torch.from_numpy(fr).to(dev)[torch.arange(n, device=dev) % F].contiguous()
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    src = torch.arange(n, dtype=torch.int64, device=dev) * P
    lens = [len(host.abf_encode(fr[k])) for k in range(F)]
    cap = sum(((lens[i % F] + 15) & ~15) for i in range(n))
    out = torch.empty((cap,), dtype=torch.uint8, device=dev)
    files = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    total = torch.zeros((1,), dtype=torch.int64, device=dev)
    scratch = torch.empty((L.abub_abf_encode_scratch_bytes(n, W, H),), dtype=torch.uint8, device=dev)
    back = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)

    def go_enc():
        _lib.check(L.abub_abf_encode_dev(frames.data_ptr(), frames.numel(), src.data_ptr(), n, W, H, out.data_ptr(), out.numel(),
                                         files.data_ptr(), total.data_ptr(), scratch.data_ptr(), scratch.numel(), stream), "enc")

    go_enc()
    torch.cuda.synchronize()
    rec = files.cpu().numpy()
    offs, flen, st = rec[:, 0], rec[:, 1] & 0xFFFFFFFF, rec[:, 1] >> 32
    assert (st == 0).all() and int(total.item()) <= cap and list(flen) == [lens[i % F] for i in range(n)]
    for k in range(0, n, max(1, n // 7)):
        assert out[offs[k]:offs[k] + flen[k]].cpu().numpy().tobytes() == host.abf_encode(fr[k % F]), k
    desc = np.zeros((n, 4), np.uint32)
    desc[:, 0], desc[:, 1] = offs, flen
    desc[:, 2], desc[:, 3] = (np.arange(n) * P) & 0xFFFFFFFF, (np.arange(n) * P) >> 32
    d_desc = torch.from_numpy(desc.view(np.int32).copy()).to(dev)

    def go_dec():
        _lib.check(L.abub_abf_decode_dev(out.data_ptr(), out.numel(), d_desc.data_ptr(), n, W, H, back.data_ptr(), back.numel(),
                                         status.data_ptr(), stream), "dec")

    go_dec()
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and torch.equal(back, frames)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    t_enc, t_dec = [], []
    for _ in range(5):
        t_enc.append(timed(go_enc))
        t_dec.append(timed(go_dec))
    ms, file_bytes = statistics.median(t_enc), int(flen.sum())
    floor_ms = (n * P / READ_CEILING_TBPS + file_bytes / FILL_CEILING_TBPS) / 1e9
    return {"frames": n, "W": W, "H": H, "packed_MB_per_frame": file_bytes / n / 1e6, "encode_ms": t_enc, "decode_ms": t_dec,
            "encode_ms_median": ms, "decode_ms_median": statistics.median(t_dec), "encode_frames_per_s": n / ms * 1e3,
            "decode_frames_per_s": n / statistics.median(t_dec) * 1e3, "encode_over_decode": ms / statistics.median(t_dec),
            "floor_ms_one_read_of_the_frames_one_write_of_the_files": floor_ms, "times_above_floor": ms / floor_ms,
            "the_encoder_reads_every_frame_twice": True, "bound_by": "not measured"}


def same_trees(a, b):
    names = lambda r: sorted(os.path.relpath(os.path.join(dp, f), r) for dp, _, fs in os.walk(r) for f in fs)  # noqa: E731
    na, nb = names(a), names(b)
    return na == nb and len(na) > 0 and all(filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False) for f in na)


def part_b(E, W=1280, H=1024, F=41, C=2):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from autobub3hs_amd import host, synth

    run_id = "20200925_0"
    tmp = tempfile.mkdtemp(prefix="abub_repack_")
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
        src = host.Run(kind="zip", run_folder=os.path.join(tmp, "png", run_id))
        res = {"host": [], "gpu": []}
        same = None
        for rep in range(3):
            dirs = {}
            for tag, device in (("host", None), ("gpu", 0)):
                dirs[tag] = os.path.join(tmp, tag, run_id)
                st = src.repack(dirs[tag], nthreads=16, ncams=C, device=device)
                res[tag].append(dict(st, frames_per_s=(st["packed"] + st["copied"]) / st["seconds"]))
            if same is None:
                same = same_trees(dirs["host"], dirs["gpu"])
            for d in dirs.values():
                shutil.rmtree(os.path.dirname(d))
        src.close()
        med = {t: statistics.median(r["frames_per_s"] for r in res[t]) for t in res}
        legs = ("read_s", "decode_s", "encode_s", "copy_s", "write_s")
        saved = 1 / PNG_READ_FPS - 1 / PACKED_READ_FPS  # seconds per frame and re-analysis
        return {"events": E, "frames": E * C * F, "runs": res, "median_frames_per_s": med, "gpu_over_host": med["gpu"] / med["host"],
                "same_trees": same,
                "gpu_route_legs_s_median": {k: statistics.median(r[k] for r in res["gpu"]) for k in legs + ("seconds",)},
                "gpu_route_batches": int(res["gpu"][0]["batches"]),
                "break_even_re_analyses": {t: 1 / med[t] / saved for t in med},
                "break_even_uses": f"reading rates {PNG_READ_FPS:.0f} (PNG zip) and {PACKED_READ_FPS:.0f} (packed) frames/s of DESIGN section 3"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "repack.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--events", type=int, default=96)
    a = ap.parse_args()

    def part_c():
        import abf_bench

        return abf_bench.part_c(a.parent)

    result = {}
    for part, fn in (("a", lambda: part_a(a.frames)), ("b", lambda: part_b(a.events)), ("c", part_c)):
        key = {"a": "kernel", "b": "end_to_end", "c": "parent_comparison"}[part]
        if part not in a.parts or (part == "c" and not a.parent):
            result[key] = "not measured"
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
