"""Bellows veto timings on one GPU, in one process, with HIP events.

1. The per-event matcher abub_match_ccorr_dev against the batched exact terms (abub_match_ccorr_batch_dev) and the
   device best match (abub_match_best_batch_dev), per job, at 1680 x 1050 with the 40l-19 template sizes 178 x 557 (cam1)
   and 152 x 509 (cam3), for batches of 1, 8 and 32 frames.
2. A pipeline run of S stacks with about 5 % of them through the veto: veto round in the batch against
   ABUB_PIPE_BELLOWS=dropin, ms per run.

    python tools/bellows_bench.py --out profiles/r04/bellows.json
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def frames_and_templates(n):
    g = os.path.join(ROOT, "tests", "golden")
    img = np.array(Image.open(os.path.join(g, "sample_40l19_cam1_image30.png")).convert("L"))
    base = np.tile(img, (1050 // img.shape[0] + 1, 1680 // img.shape[1] + 1))[:1050, :1680]
    rng = np.random.RandomState(3)
    fr = np.stack([np.clip(base.astype(int) + rng.randint(-4, 5, base.shape), 0, 255) for _ in range(n)]).astype(np.uint8)
    t = Image.open(os.path.join(g, "sample_40l19_cam1_bellows_template.png")).convert("L")
    return fr, {"178x557": np.array(t.resize((178, 557))), "152x509": np.array(t.resize((152, 509)))}


def timed(fn, reps):
    import torch

    fn()  # warm-up (code object load)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out)), out


def kernels(res, reps):
    import torch

    from autobub3hs_amd import _lib, hip

    dev = "cuda:0"
    fr, tpls = frames_and_templates(32)
    d_fr = torch.from_numpy(fr).to(dev)
    H, W = fr.shape[1:]
    st = torch.cuda.current_stream().cuda_stream
    for name, t in tpls.items():
        th, tw = t.shape
        d_t = torch.from_numpy(t).to(dev)
        rh, rw = H - th + 1, W - tw + 1
        num = torch.empty((rh, rw), dtype=torch.int64, device=dev)
        w2 = torch.empty_like(num)
        old_ms, old_all = timed(lambda: _lib.check(_lib.lib().abub_match_ccorr_dev(
            d_fr[0].data_ptr(), W, H, d_t.data_ptr(), tw, th, num.data_ptr(), w2.data_ptr(), st)), reps)
        row = {"template": name, "macs_per_job": rw * rh * tw * th, "old_ccorr_ms_per_job": old_ms, "old_all": old_all,
               "batches": []}
        for nb in (1, 8, 32):
            idx = torch.arange(nb, dtype=torch.int32, device=dev)
            terms_ms, _ = timed(lambda: hip.match_terms(d_fr, idx, d_t), reps)
            scratch = torch.empty(_lib.lib().abub_match_best_scratch_bytes(W, H, tw, th, nb), dtype=torch.uint8, device=dev)
            best_ms, _ = timed(lambda: hip.match_best(d_fr, idx, d_t, scratch), reps)
            row["batches"].append({"jobs": nb, "terms_ms_per_job": terms_ms / nb, "best_ms_per_job": best_ms / nb,
                                   "best_speedup_vs_old": old_ms / (best_ms / nb)})
        res["kernels"].append(row)
        print(json.dumps(row), flush=True)


def pipeline(res, reps, E):
    import torch

    from autobub3hs_amd import hip, host, synth
    from test_bellows_batched import bellows_event, write_bmp8

    dev = "cuda:0"
    W, H, F, t0 = 200, 120, 24, 12
    fr, tex, (bx0, by0) = bellows_event(W, H, F, t0, shift=2)
    tr = synth.training_pairs(W, H, 8, 0, F)
    for k in range(len(tr)):
        tr[k, by0:by0 + 50, bx0:bx0 + 30] = tex
    d_tr = torch.from_numpy(tr).to(dev)
    mu, sg = hip.train(d_tr, W, H)
    out = tempfile.mkdtemp(prefix="bellows_masks_")
    bel = np.zeros((H, W), np.uint8)
    bel[by0 - 10:by0 + 60, bx0 - 10:bx0 + 45] = 255
    write_bmp8(os.path.join(out, "cam0_bellows_mask.bmp"), bel)
    Image.fromarray(tex).save(os.path.join(out, "cam0_bellows_template.png"))
    stacks = []
    for e in range(E):
        if e % 20 == 0:
            stacks.append(fr)  # 5 % through the veto
        else:
            stacks.append(synth.render_event(W, H, synth.EventSpec(F, t0=10, bubbles=[(60, 60, 40)]), 100 + e, 0))
    d_slab = torch.from_numpy(np.ascontiguousarray(np.stack(stacks)[:, None])).to(dev)
    s6 = hip.sigma6(sg[None].contiguous())
    rows = {}
    for mode in ("batched", "dropin"):
        if mode == "dropin":
            os.environ["ABUB_PIPE_BELLOWS"] = "dropin"
        pipe = host.Pipeline(0, W, H, F, E, 1, [len(tr)], nthreads=16, maskdir=out)
        os.environ.pop("ABUB_PIPE_BELLOWS", None)
        st = torch.cuda.current_stream().cuda_stream

        def go():
            pipe.run(d_slab, mu[None].contiguous(), s6, st, sigma=sg[None].contiguous())

        ms, allv = timed(go, reps)
        rows[mode] = {"ms_per_run": ms, "all": allv, "timing": pipe.timing(), "bellows": pipe.bellows_stats(),
                      "summary": pipe.summary()}
        pipe.close()
    assert rows["batched"]["summary"] == rows["dropin"]["summary"], "the two routes disagree"
    for r in rows.values():
        del r["summary"]
    res["pipeline"] = {"stacks": E, "vetoed_share": sum(1 for e in range(E) if e % 20 == 0) / E, "W": W, "H": H, "F": F,
                       **rows, "speedup": rows["dropin"]["ms_per_run"] / rows["batched"]["ms_per_run"]}
    print(json.dumps(res["pipeline"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stacks", type=int, default=200)
    a = ap.parse_args()
    import torch

    from autobub3hs_amd import host

    host.build()
    res = {"device": torch.cuda.get_device_name(0), "kernels": []}
    kernels(res, a.reps)
    pipeline(res, a.reps, a.stacks)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
