"""The numpy restatement of a survey ("Surveying a run"): the per-frame record of abub_frame_stats_dev /
frameStatsHost, the pairing of the frames of a stack, and the report's text.  Nothing here calls the code under test."""
import math

import numpy as np

KEYS = ("min", "max", "n_zero", "n_sat", "n_out", "n_moved", "flags", "sum", "sumsq", "sum_out", "sum_moved")
COLUMNS = ("status",) + KEYS  # of hip.frame_stats
F_MODEL, F_REF = 1, 2
E_RANGE = 1
HEADER = "event\tcam\tframe\tname\tstate\tw\th\tmin\tmax\tsum\tsumsq\tn_zero\tn_sat\tn_out\tsum_out\tn_moved\tsum_moved\tmean\tsd\n"


def sigma6_of(sigma):
    return np.minimum(np.asarray(sigma).astype(np.int64) * 6, 255).astype(np.uint8)


def record(cur, ref=None, mu=None, sigma6=None):
    """the record of one frame: dict of KEYS, every value a Python int"""
    p = np.asarray(cur, np.uint8).reshape(-1).astype(np.int64)
    rec = dict(min=int(p.min()), max=int(p.max()), n_zero=int((p == 0).sum()), n_sat=int((p == 255).sum()), n_out=0, n_moved=0,
               flags=0, sum=int(p.sum()), sumsq=int((p * p).sum()), sum_out=0, sum_moved=0)
    if mu is None:
        return rec
    s = np.asarray(sigma6, np.uint8).reshape(-1).astype(np.int64)
    out = np.maximum(np.abs(p - np.asarray(mu, np.uint8).reshape(-1).astype(np.int64)) - s, 0)
    rec.update(flags=F_MODEL, n_out=int((out > 0).sum()), sum_out=int(out.sum()))
    if ref is not None:
        moved = np.maximum(np.abs(p - np.asarray(ref, np.uint8).reshape(-1).astype(np.int64)) - s, 0)
        rec.update(flags=F_MODEL | F_REF, n_moved=int((moved > 0).sum()), sum_moved=int(moved.sum()))
    return rec


def kernel_row(rec):
    """a record as a row of hip.frame_stats (status 0 in front)"""
    return [0] + [rec[k] for k in KEYS]


RANGE_ROW = [E_RANGE] + [0] * len(KEYS)


def model_line(cam, model):
    """model: None, or dict(trained=TrainingSetSize, mu=[H, W] u8, sigma=[H, W] u8)"""
    if model is None:
        return f"model cam {cam} none\n"
    sg = np.asarray(model["sigma"]).astype(np.int64)
    return (f"model cam {cam} trained {model['trained']} sigma_zero {int((sg == 0).sum())} sigma6_sat {int((6 * sg >= 255).sum())} "
            f"sigma_max {int(sg.max())} mu_mean {int(np.asarray(model['mu']).astype(np.int64).sum()) / sg.size:.6f}\n")


def rows_of(stacks, W, H, models):
    """stacks: [(event, cam, [(name, image or None)])] in report order, every stack's frames in name order; image: a u8
    array (ok when it is H x W, else other_size), None (undecodable) or the string "missing" -> the report's rows"""
    rows = []
    for event, cam, frames in stacks:
        model = models[cam]
        for i, (name, img) in enumerate(frames):
            row = dict(event=str(event), cam=cam, frame=i, name=name, rec=None, w=0, h=0)
            if isinstance(img, str):
                row["state"] = "missing"
            elif img is None:
                row["state"] = "undecodable"
            elif img.shape != (H, W):
                row.update(state="other_size", h=img.shape[0], w=img.shape[1], rec=record(img))
            else:
                ref = frames[max(i - 2, 0)][1]
                ref = ref if isinstance(ref, np.ndarray) and ref.shape == (H, W) else None
                row.update(state="ok", h=H, w=W)
                row["rec"] = record(img) if model is None else record(img, ref, model["mu"], sigma6_of(model["sigma"]))
            rows.append(row)
    return rows


def report(models, rows):
    text = "# abub3hs survey 1\n" + "".join(model_line(c, m) for c, m in enumerate(models)) + HEADER
    shares = []
    for r in rows:
        text += f"{r['event']}\t{r['cam']}\t{r['frame']}\t{r['name']}\t{r['state']}"
        rec = r["rec"]
        if rec is None:
            text += "\t-" * 14 + "\n"
            continue
        n = r["w"] * r["h"]
        text += f"\t{r['w']}\t{r['h']}\t{rec['min']}\t{rec['max']}\t{rec['sum']}\t{rec['sumsq']}\t{rec['n_zero']}\t{rec['n_sat']}"
        ok = r["state"] == "ok"
        text += f"\t{rec['n_out']}\t{rec['sum_out']}" if ok and rec["flags"] & F_MODEL else "\t-\t-"
        if ok and rec["flags"] & F_REF:
            text += f"\t{rec['n_moved']}\t{rec['sum_moved']}"
            shares.append(rec["n_moved"] / float(n))
        else:
            text += "\t-\t-"
        mean = rec["sum"] / float(n)
        text += f"\t{mean:.6f}\t{math.sqrt(max(0.0, rec['sumsq'] / float(n) - mean * mean)):.6f}\n"
    count = {s: sum(1 for r in rows if r["state"] == s) for s in ("ok", "undecodable", "missing", "other_size")}
    text += (f"run frames {len(rows)} ok {count['ok']} undecodable {count['undecodable']} missing {count['missing']} "
             f"other_size {count['other_size']}")
    pixels = sum(np.asarray(m["sigma"]).size for m in models if m is not None)
    zero = sum(int((np.asarray(m["sigma"]) == 0).sum()) for m in models if m is not None)
    text += f" sigma_zero_share {zero / float(pixels):.6f}" if pixels else " sigma_zero_share -"
    if shares:
        shares.sort()
        k = len(shares)
        text += f" moved_share_median {shares[k // 2] if k & 1 else (shares[k // 2 - 1] + shares[k // 2]) / 2:.6f}\n"
    else:
        text += " moved_share_median -\n"
    return text
