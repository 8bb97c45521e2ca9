"""Interleaved A/B of the pipeline's "localize" knob on bench.py's synthetic run in each data regime: contours 1 (K5 ships
the polygons, stage 4 runs LocalizeOMatic's arithmetic and decisions per stack on host threads) against localize 1 (K7,
abub_localize.hip: the device describes the contours and decides; stage 4 rebuilds the bubbles from finished tracks), with
the "trigger" knob at 0 and at 1, for each host thread count.

One pipeline object per (regime, thread count); steps cycle through the four settings on it (A B C D A B C D ...), each
step timed from a device synchronise to the end of the run (the pipeline synchronises itself).  Per step: ms, the
pipeline's stage timings, rounds and localize_stats() (K7 ms, stacks on the host route, list bytes shipped).  Results must
not depend on the knobs: every step's per-stack summary is compared.  2 threads are the host share of one rank of an
8-GPU node.

    python tools/localize_ab.py --steps 8 --threads 16,2 --out profiles/r07/localize_ab.json
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
    ap.add_argument("--steps", type=int, default=8, help="steps per setting (interleaved)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--events", type=int, default=100)
    ap.add_argument("--cams", type=int, default=2)
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--threads", default="16,2")
    ap.add_argument("--regimes", default="default,post_trigger_dense,noisy")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from autobub3hs_amd import hip, host, synth

    if not torch.cuda.is_available():
        raise SystemExit("localize_ab.py needs a GPU")
    dev = "cuda:0"
    W, H, F, E, C = args.width, args.height, args.frames, args.events, args.cams
    maskdir = tempfile.mkdtemp(prefix="abub_masks_") + "/"
    accept_for = synth.write_masks(maskdir, W, H, C)
    bgs = [synth.background(W, H, synth.BASE_SEED + c, "torch", dev) for c in range(C)]
    out = {"config": {"W": W, "H": H, "F": F, "E": E, "C": C, "steps": args.steps, "device": torch.cuda.get_device_name(0)},
           "runs": []}
    settings = (("t0l0", 0, 0), ("t0l1", 0, 1), ("t1l0", 1, 0), ("t1l1", 1, 1))
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
        stream = torch.cuda.current_stream().cuda_stream
        for threads in [int(t) for t in args.threads.split(",")]:
            pipe = host.Pipeline(0, W, H, F, E, C, [2 * min(4, E)] * C, nthreads=threads, maskdir=maskdir)
            pipe.set_sigma(sg_t)
            rows, ref = [], None
            for k in range(len(settings) * (args.warmup + args.steps)):
                name, vt, vl = settings[k % len(settings)]
                pipe.set_option("trigger", vt)
                pipe.set_option("contours", 1)
                pipe.set_option("localize", vl)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.run(slab, mu_t, s6, stream)
                ms = (time.perf_counter() - t0) * 1e3
                summ = pipe.summary()
                if ref is None:
                    ref = summ
                assert summ == ref, "results depend on the trigger / localize knobs"
                if k < len(settings) * args.warmup:
                    continue
                t = pipe.timing()
                row = {"setting": name, "trigger": vt, "localize": vl, "ms": ms, "rounds": t["rounds"]}
                row.update({k_: t[k_] for k_ in ("stage1_ms", "stage2_ms", "stage3_ms", "stage4_ms")})
                row.update({"loc_" + k_: v for k_, v in pipe.localize_stats().items()})
                row["k5_ms"] = pipe.contour_stats()["k5_ms"]
                rows.append(row)
            pipe.close()
            summary = {}
            for name, _, _ in settings:
                mine = [r for r in rows if r["setting"] == name]
                summary[name] = {k_: statistics.median(r[k_] for r in mine) for k_ in mine[0] if k_ != "setting"}
            # the medians carry the result; of the single steps only the times are kept, in the order they ran
            step_ms = {name: [round(r["ms"], 4) for r in rows if r["setting"] == name] for name, _, _ in settings}
            out["runs"].append({"regime": regime, "threads": threads, "summary": summary, "step_ms": step_ms})
            print(regime, threads, json.dumps(summary), flush=True)
        del slab
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("{\n \"config\": %s,\n \"runs\": [\n  %s\n ]\n}\n"
                    % (json.dumps(out["config"]), ",\n  ".join(json.dumps(r) for r in out["runs"])))


if __name__ == "__main__":
    main()
