"""The numpy restatement of a survey's per-cell noise records ("Surveying a run for noise changes"): the six
words of abub_frame_noise_cells_dev / noiseCellsHost, which rows have a record, the baseline a camera's rows at stack
position 1 give, what a cell and a frame say, noise.txt and the arrays of the .npy files.  int64 sums and Python integers;
nothing here calls the code under test.  The grid is the field's (fieldref.grid), restated there."""
import numpy as np

from fieldref import CELL, grid  # noqa: F401
from lightref import _cells, sigma6_of  # noqa: F401

N = CELL * CELL
E_RANGE = 1
NOISY_MILLI, QUIET_MILLI = 1500, 667
HEADER = "event\tcam\tframe\tname\tstate\tindex\trated\tclipped\tbusy\tnoisy\tquiet\tq_milli\tq_min\tq_max\tall_milli\tkind\n"
KINDS = ("blind", "busy", "steady", "noisy", "quiet", "uneven")


def records(p, r, sigma6, x0, y0, ncx, ncy):
    """p, r, sigma6: u8 [H, W] -> int32 [ncy, ncx, 6]: n_over, n_clip, s1_in, s2_in, sad, s2_all of d = p - r"""
    p, r, s = (_cells(a, x0, y0, ncx, ncy) for a in (p, r, sigma6))
    d = p - r
    over = np.abs(d) > s
    clip = (p == 0) | (p == 255) | (r == 0) | (r == 255)
    parts = [over, clip, np.where(over, 0, d), np.where(over, 0, d * d), np.abs(d), d * d]
    out = np.stack([q.sum(axis=(1, 3), dtype=np.int64) for q in parts], axis=-1)
    assert np.abs(out).max() <= N * 255 * 255 < 2 ** 31
    return out.astype(np.int32)


def n_in(rec):
    return N - int(rec[0])


def energy(rec):
    """E: the inside sum of squares about the inside mean"""
    n = n_in(rec)
    return int(rec[3]) - int(rec[2]) ** 2 // n if n > 0 else 0


def clipped(rec):
    return int(rec[1]) * 8 > N


def busy(rec):
    return int(rec[0]) * 4 > N


def model_records(sigma6, base, x0, y0, ncx, ncy):
    """sigma6: u8 [H, W]; base: the records [ncy, ncx, 6] of the camera's rows at stack position 1 that have one
    -> int64 [ncy, ncx, 5]: BE, BN, B, sum s^2, pixels with s == 0"""
    s = _cells(sigma6, x0, y0, ncx, ncy)
    out = np.zeros((ncy, ncx, 5), np.int64)
    out[..., 3] = (s * s).sum(axis=(1, 3))
    out[..., 4] = (s == 0).sum(axis=(1, 3))
    for cy in range(ncy):
        for cx in range(ncx):
            for rec in base:
                r = np.asarray(rec)[cy, cx]
                if not clipped(r) and not busy(r):
                    out[cy, cx, 0] += energy(r)
                    out[cy, cx, 1] += n_in(r)
                    out[cy, cx, 2] += 1
    return out


def model_milli(model):
    BE, BN, ss = int(model[0]), int(model[1]), int(model[3])
    return 1000 * 18 * BE * N // (BN * ss) if BN > 0 and ss > 0 else 0


def cell(rec, model):
    """-> dict(state: clipped, busy, nobase, noisy, quiet or same; q_milli (None unless rated), all_milli)"""
    BE, BN, B = int(model[0]), int(model[1]), int(model[2])
    base = BE > 0 and B > 0
    out = dict(q_milli=None, all_milli=1000 * int(rec[5]) * BN // (N * BE) if base else 0)
    if clipped(rec):
        out["state"] = "clipped"
    elif busy(rec):
        out["state"] = "busy"
    elif not base:
        out["state"] = "nobase"
    else:
        q = out["q_milli"] = 1000 * energy(rec) * BN // (n_in(rec) * BE)
        out["state"] = "noisy" if q > NOISY_MILLI else "quiet" if q < QUIET_MILLI else "same"
    return out


def rated(c):
    return c["state"] in ("noisy", "quiet", "same")


def summary(rec, model):
    """rec [ncy, ncx, 6], model [ncy, ncx, 5] -> dict(rated, clipped, busy, noisy, quiet, q_milli, q_min, q_max (None: `-`),
    all_milli, kind, changed_cells: bool [ncy, ncx])"""
    rec, model = np.asarray(rec), np.asarray(model)
    shape = rec.shape[:-1]
    recs, mods = rec.reshape(-1, 6), model.reshape(-1, 5)
    cells = [cell(r, m) for r, m in zip(recs, mods)]
    on = [k for k, c in enumerate(cells) if rated(c)]
    count = lambda s: sum(c["state"] == s for c in cells)  # noqa: E731
    out = dict(rated=len(on), clipped=count("clipped"), busy=count("busy"), noisy=count("noisy"), quiet=count("quiet"), q_milli=None,
               q_min=None, q_max=None, all_milli=0,
               changed_cells=np.array([c["state"] in ("noisy", "quiet") for c in cells], bool).reshape(shape))
    if on:
        num = sum(energy(recs[k]) * int(mods[k][1]) for k in on)
        den = sum(n_in(recs[k]) * int(mods[k][0]) for k in on)
        out["q_milli"] = 1000 * num // den
        out["q_min"], out["q_max"] = min(cells[k]["q_milli"] for k in on), max(cells[k]["q_milli"] for k in on)
    based = [k for k, c in enumerate(cells) if c["state"] != "clipped" and int(mods[k][0]) > 0 and int(mods[k][2]) > 0]
    if based:
        out["all_milli"] = 1000 * sum(int(recs[k][5]) * int(mods[k][1]) for k in based) // sum(N * int(mods[k][0]) for k in based)
    U = len(cells) - out["clipped"]
    if (out["rated"] + out["busy"]) * 4 < len(cells):
        out["kind"] = "blind"
    elif out["busy"] * 2 > U:
        out["kind"] = "busy"
    elif not out["noisy"] and not out["quiet"]:
        out["kind"] = "steady"
    elif not out["quiet"] and out["noisy"] * 2 >= out["rated"]:
        out["kind"] = "noisy"
    elif not out["noisy"] and out["quiet"] * 2 >= out["rated"]:
        out["kind"] = "quiet"
    else:
        out["kind"] = "uneven"
    return out


def rows_of(stacks, W, H, models, R):
    """stacks: [(event, cam, [(name, image or None or "missing")])] as surveyref.rows_of takes them; models[cam]: None or
    dict(mu=, sigma=) -> noise.txt's rows: dicts with event, cam, frame, name, state and rec (None: no record).  Frame i of a
    stack is paired with frame max(i - 2, 0) of it: a record needs an ok row of a camera with a model whose reference is
    another row, ok as well"""
    ncx, ncy, x0, y0 = grid(W, H, R)
    ok = lambda img: not isinstance(img, str) and img is not None and img.shape == (H, W)  # noqa: E731
    rows = []
    for event, cam, frames in stacks:
        for i, (name, img) in enumerate(frames):
            row = dict(event=str(event), cam=cam, frame=i, name=name, rec=None)
            if isinstance(img, str):
                row["state"] = "missing"
            elif img is None:
                row["state"] = "undecodable"
            elif img.shape != (H, W):
                row["state"] = "other_size"
            else:
                row["state"] = "ok"
                ref = max(i - 2, 0)
                if models[cam] is not None and ref != i and ok(frames[ref][1]):
                    row["rec"] = records(img, frames[ref][1], sigma6_of(models[cam]["sigma"]), x0, y0, ncx, ncy)
            rows.append(row)
    return rows


def model_arrays(models, rows, W, H, R):
    """-> {cam: int64 [ncy, ncx, 5]} for every camera with a model: what cam<c>_noise_model.npy holds"""
    ncx, ncy, x0, y0 = grid(W, H, R)
    return {c: model_records(sigma6_of(m["sigma"]), [r["rec"] for r in rows if r["cam"] == c and r["frame"] == 1 and r["rec"] is not None],
                             x0, y0, ncx, ncy) for c, m in enumerate(models) if m is not None}


def arrays(models, rows, W, H, R):
    """-> {cam: int32 [N_c, ncy, ncx, 6]} for every camera with a model: what cam<c>_noise.npy holds"""
    ncx, ncy, _, _ = grid(W, H, R)
    out = {}
    for c, m in enumerate(models):
        if m is not None:
            mine = [r["rec"] for r in rows if r["cam"] == c and r["rec"] is not None]
            out[c] = np.array(mine, np.int64).astype(np.int32).reshape(len(mine), ncy, ncx, 6)
    return out


def report(models, rows, W, H, R):
    ncx, ncy, x0, y0 = grid(W, H, R) if W > 0 else (0, 0, 0, 0)
    text = f"# abub3hs noise 1\nradius {R} cell {CELL} grid {ncx} {ncy} origin {x0} {y0}\n" + HEADER
    mrec = model_arrays(models, rows, W, H, R)
    index = [0] * len(models)
    per_cam = [dict(frames=0, first="-", changed=np.zeros((ncy, ncx), np.int64), **{k: 0 for k in KINDS}) for _ in models]
    dash = lambda v: "-" if v is None else str(v)  # noqa: E731
    for r in rows:
        text += f"{r['event']}\t{r['cam']}\t{r['frame']}\t{r['name']}\t{r['state']}"
        if r["rec"] is None:
            text += "\t-" * 11 + "\n"
            continue
        s, c = summary(r["rec"], mrec[r["cam"]]), per_cam[r["cam"]]
        text += f"\t{index[r['cam']]}" + "".join(f"\t{s[k]}" for k in ("rated", "clipped", "busy", "noisy", "quiet"))
        index[r["cam"]] += 1
        text += "".join("\t" + dash(s[k]) for k in ("q_milli", "q_min", "q_max")) + f"\t{s['all_milli']}\t{s['kind']}\n"
        c["frames"] += 1
        c[s["kind"]] += 1
        c["changed"] += s["changed_cells"]
        if s["noisy"] + s["quiet"] and c["first"] == "-":
            c["first"] = r["event"]
    for c, m in enumerate(models):
        if m is None:
            text += f"noise cam {c} none\n"
        else:
            k = per_cam[c]
            text += (f"noise cam {c} frames {k['frames']} " + " ".join(f"{q} {k[q]}" for q in KINDS) + f" first_changed_event {k['first']}"
                     + " model_milli" + "".join(f" {model_milli(v)}" for v in mrec[c].reshape(-1, 5)) + "\n")
    for c, m in enumerate(models):
        if m is not None:
            for y in range(ncy):
                text += f"changed cam {c} y {y}" + "".join(f" {int(v)}" for v in per_cam[c]["changed"][y]) + "\n"
    total = {q: sum(per_cam[c][q] for c, m in enumerate(models) if m is not None) for q in ("frames",) + KINDS}
    return text + f"run frames {total['frames']} " + " ".join(f"{q} {total[q]}" for q in KINDS) + "\n"
