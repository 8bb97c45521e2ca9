"""Interleaved A/B of the pipeline's "blobs" and "contours" knobs on bench.py's synthetic run in each data regime:
blobs0 (the host applies the Otsu cut to every candidate pixel and traces the contours), blobs1 (the GPU labels the
foreground and ships only the kept pixels; the host traces them), contours1 (the GPU also traces the contours, K5, and
ships their vertices).

One pipeline object per regime; steps cycle through the three settings on it (A B C A B C ...), each step timed from a
device synchronise to the end of the run (the pipeline synchronises itself).  Per step: ms, the pipeline's stage timings
and, with a knob on, blob_stats() / contour_stats().  Results must not depend on the knobs: every step's per-stack summary
is compared.  --threads 2 is the host share of one rank of an 8-GPU node.

    python tools/blob_ab.py --steps 10 --out profiles/r05/contours_ab_t16.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="steps per setting and regime (interleaved)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--events", type=int, default=100)
    ap.add_argument("--cams", type=int, default=2)
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--regimes", default="default,post_trigger_dense,noisy")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from autobub3hs_amd import hip, host, synth

    if not torch.cuda.is_available():
        raise SystemExit("blob_ab.py needs a GPU")
    dev = "cuda:0"
    W, H, F, E, C = args.width, args.height, args.frames, args.events, args.cams
    maskdir = tempfile.mkdtemp(prefix="abub_masks_") + "/"
    accept_for = synth.write_masks(maskdir, W, H, C)
    bgs = [synth.background(W, H, synth.BASE_SEED + c, "torch", dev) for c in range(C)]
    out = {"config": {"W": W, "H": H, "F": F, "E": E, "C": C, "threads": args.threads, "steps": args.steps,
                      "device": torch.cuda.get_device_name(0)}, "regimes": {}}
    for regime in args.regimes.split(","):
        slab = torch.empty((E * C, F, H, W), dtype=torch.uint8, device=dev)
        for e in range(E):
            for c in range(C):
                spec = synth.random_spec(W, H, F, e, c, p_second=0.2, accept=accept_for(c), regime=regime)
                synth.render_event(W, H, spec, e, c, xp="torch", device=dev, out=slab[e * C + c], bg=bgs[c])
        mus, sgs = [], []
        for c in range(C):
            idx = torch.tensor([((e * C + c) * F + f) for e in range(min(4, E)) for f in (0, 1)], dtype=torch.int32, device=dev)
            mu, sg = hip.train(slab, W, H, idx=idx)
            mus.append(mu)
            sgs.append(sg)
        mu_t, sg_t = torch.stack(mus).contiguous(), torch.stack(sgs).contiguous()
        s6 = hip.sigma6(sg_t)
        pipe = host.Pipeline(0, W, H, F, E, C, [2 * min(4, E)] * C, nthreads=args.threads, maskdir=maskdir)
        pipe.set_sigma(sg_t)
        stream = torch.cuda.current_stream().cuda_stream
        rows, ref = [], None
        settings = (("blobs0", 0, 0), ("blobs1", 1, 0), ("contours1", 0, 1))
        for k in range(len(settings) * (args.warmup + args.steps)):
            name, vb, vc = settings[k % len(settings)]
            pipe.set_option("blobs", vb)
            pipe.set_option("contours", vc)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.run(slab, mu_t, s6, stream)
            ms = (time.perf_counter() - t0) * 1e3
            summ = pipe.summary()
            if ref is None:
                ref = summ
            assert summ == ref, "results depend on the blobs / contours knobs"
            if k < len(settings) * args.warmup:
                continue
            t = pipe.timing()
            row = {"setting": name, "blobs": vb, "contours": vc, "ms": ms, "stage3_ms": t["stage3_ms"],
                   "stage4_ms": t["stage4_ms"], "s3_gpu_ms": t["s3_gpu_ms"], "s3_list_ms": t["s3_list_ms"], "pairs": t["pairs"]}
            if vb or vc:
                row["blob_stats"] = pipe.blob_stats()
            if vc:
                row["contour_stats"] = pipe.contour_stats()
            rows.append(row)
        pipe.close()
        del slab

        summary = {}
        for name, _, _ in settings:
            mine = [r for r in rows if r["setting"] == name]
            summary[name] = {k: statistics.median(r[k] for r in mine)
                             for k in ("ms", "stage3_ms", "stage4_ms", "s3_gpu_ms", "s3_list_ms")}
            for key in ("blob_stats", "contour_stats"):
                b = [r[key] for r in mine if key in r]
                if b:
                    summary[name].update({k: statistics.median(x[k] for x in b) for k in b[0]})
        # what travels to the host per step: every candidate pair (5 bytes: index + value), the kept indices (4 bytes), the
        # contour vertices (4 bytes) plus the kept indices of the batches with a declined slot
        summary["shipped"] = {"blobs0_pixels": summary["blobs1"]["candidates"], "blobs1_pixels": summary["blobs1"]["kept"],
                              "contours1_vertices": summary["contours1"]["vertices"],
                              "contours1_host_route_slots": summary["contours1"]["host_route"]}
        out["regimes"][regime] = {"summary": summary, "steps": rows}
        print(regime, json.dumps(summary), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
