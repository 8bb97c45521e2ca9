#!/usr/bin/env python3
"""Interlaced PNG on the GPU ("Interlaced PNG") measured on one GPU box -> profiles/r17/adam7.json.
  (a) kernel: 1024 resident 1280x1024 synth frames written Adam7-interlaced as 8-bit grey and as RGB 8 (tests/pngadam7.py;
      row r of pass p carries the filter type Pillow chose for that image row in the non-interlaced file of the same image):
      abub_png_decode_adam7_dev on each, next to the existing entries (abub_png_decode_dev, abub_png_decode_typed_dev) on the
      same images written without interlace by the same writer with the same filter types and the same zlib level, five
      alternating launches each after a warm-up, device events, medians; and 16 host threads decoding the same files
      (host.imdecode).  The parent commit cannot read the interlaced files: there is no parent leg;
  (b) nothing else moved: bench.py --steps 20 --warmup 5, a built checkout of the parent commit (--parent DIR) and this tree
      alternating (--order, T: this tree, P: the parent), the dumped outputs compared.
usage: python3 tools/adam7_bench.py [--parts ab] [--parent DIR] [--out profiles/r17/adam7.json] [--frames 1024] [--order TPPTTP]"""
import argparse, json, os, statistics, sys, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402


def files_of(fr, nthr):
    """-> {name: (files, kind bits)} for the frames fr [F, H, W]: grey8 / rgb8, each interlaced ("_adam7") and not"""
    from concurrent.futures import ThreadPoolExecutor
    import pngadam7 as a7
    import pngtypes as pt
    from png_types_bench import filter_types_of, pillow_png

    F, H, W = fr.shape

    def one(k):
        out = {}
        for name, ctype, S in (("grey8", 0, 1), ("rgb8", 2, 3)):
            s = np.repeat(fr[k][:, :, None], S, axis=2).astype(np.uint16)
            fts = filter_types_of(pillow_png(s[:, :, 0].astype(np.uint8) if S == 1 else s.astype(np.uint8)), W, H, S * W)
            out[name] = pt.make_png(s, ctype, 8, fts)
            out[name + "_adam7"] = a7.make_adam7(s, ctype, 8, lambda p, r: fts[a7.PASSES[p][1] + r * a7.PASSES[p][3]])
        return out

    with ThreadPoolExecutor(nthr) as ex:
        per = list(ex.map(one, range(F)))
    return {name: [p[name] for p in per] for name in per[0]}


class Resident:
    """n files on the device with their descriptors: one launch per go(); mode: plain, typed or adam7 (the entry)"""

    def __init__(self, files, W, H, mode):
        import torch
        from autobub3hs_amd import hip, _lib

        self.L, self.W, self.H, self.mode, self.n = _lib.lib(), W, H, mode, len(files)
        n, P = self.n, W * H
        rec = np.zeros((n, 8), dtype=np.uint32)
        segs, blob, zoff = [], bytearray(), 0
        self.stride = int(self.L.abub_png_raw_stride(W, H))
        for i, data in enumerate(files):
            sg, lut, kind = hip.png_parse(data, W, H, types=True, adam7=True)
            assert lut is None and ((kind & hip.PNG_KIND_ADAM7) != 0) == (mode == "adam7") and (mode != "plain" or kind == 0)
            self.stride = max(self.stride, int(self.L.abub_png_raw_stride_adam7(W, H, kind)))
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
        if self.mode == "adam7":
            _lib.check(self.L.abub_png_decode_adam7_dev(*a, self.stride, *b), "abub_png_decode_adam7_dev")
        elif self.mode == "typed":
            _lib.check(self.L.abub_png_decode_typed_dev(*a, self.stride, *b), "abub_png_decode_typed_dev")
        else:
            _lib.check(self.L.abub_png_decode_dev(*a, *b), "abub_png_decode_dev")


def part_a(n, W=1280, H=1024):
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from autobub3hs_amd import host, synth

    F = 41
    nthr = min(16, len(os.sched_getaffinity(0)))
    fr = np.asarray(synth.render_event(W, H, synth.random_spec(W, H, F, 3, 0), 3, 0))
    t0 = time.perf_counter()
    kinds = files_of(fr, nthr)
    res = {"frames": n, "W": W, "H": H, "files_made_in_s": time.perf_counter() - t0, "kinds": {}}
    mode = {"grey8": "plain", "rgb8": "typed", "grey8_adam7": "adam7", "rgb8_adam7": "adam7"}
    runs, count = {}, {}
    for name, files in kinds.items():
        count[name] = min(n, int(3.6e9 // (max(len(f) for f in files) + 64)) // 64 * 64)  # (a launch takes less than 4 GB of files)
        r = Resident([files[i % F] for i in range(count[name])], W, H, mode[name])
        r.go()  # warm-up, and the check
        torch.cuda.synchronize()
        assert (r.status.cpu().numpy() == 0).all(), name
        for k in range(0, count[name], max(1, count[name] // 7)):
            assert np.array_equal(r.out[k].cpu().numpy(), fr[k % F]), (name, k)
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
    for name, files in kinds.items():
        nk = count[name]
        batch = [files[i % F] for i in range(nk)]
        with ThreadPoolExecutor(nthr) as ex:
            list(ex.map(host.imdecode, batch[:nthr]))
            t0 = time.perf_counter()
            got = list(ex.map(lambda d: host.imdecode(d, cap=W * H), batch))
            dt = time.perf_counter() - t0
        assert np.array_equal(got[5], fr[5])
        med = statistics.median(ms[name])
        res["kinds"][name] = {"frames": nk, "MB_per_file": runs[name].file_bytes / nk / 1e6, "raw_stride_bytes": runs[name].stride,
                              "ms": ms[name], "ms_median": med, "gpu_frames_per_s": nk / med * 1e3, "host_threads": nthr,
                              "host_frames_per_s": nk / dt, "gpu_over_host": nk / med * 1e3 / (nk / dt)}
    for name in ("grey8", "rgb8"):
        a, b = res["kinds"][name + "_adam7"], res["kinds"][name]
        a["gpu_interlaced_over_non_interlaced"] = a["gpu_frames_per_s"] / b["gpu_frames_per_s"]
        a["host_interlaced_over_non_interlaced"] = a["host_frames_per_s"] / b["host_frames_per_s"]
    del runs
    torch.cuda.empty_cache()
    return res


def part_b(parent, order):
    import verify_bench

    return verify_bench.part_c_balanced(parent, order)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ab")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "adam7.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--order", default="TPPTTP")
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):  # (a part measured by an earlier call stays)
        result = json.load(open(a.out))
    # (a series in another order than the default is kept next to it, e.g. --order TPPTTPPTTPPT)
    key_b = "parent_comparison" if a.order == ap.get_default("order") else "parent_comparison_" + a.order
    parts = (("a", "kernel", lambda: part_a(a.frames)), ("b", key_b, lambda: part_b(os.path.abspath(a.parent), a.order)))
    for part, key, fn in parts:
        if part not in a.parts or (part == "b" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
