"""The numpy restatement of a survey's per-cell light records ("Surveying a run for lighting changes"): the
six sums of abub_frame_light_cells_dev / lightCellsHost, the model's three, rdiv, what a cell and a frame say, the pairing of
the rows with their camera's model, light.txt and the arrays of the .npy files.  int64 sums and Python integers; nothing here
calls the code under test.  The grid is the field's (fieldref.grid), restated there."""
import numpy as np

from fieldref import CELL, grid  # noqa: F401

N = CELL * CELL
E_RANGE = 1
HEADER = ("event\tcam\tframe\tname\tstate\tindex\trated\tclipped\tchanged\tup\tdown\tlevel_milli\tratio_min\tratio_max\tgain_milli\t"
          "offset_milli\tkind\n")
KINDS = ("blind", "steady", "level", "uneven")


def _cells(a, x0, y0, ncx, ncy):
    """[H, W] -> int64 [ncy, 128, ncx, 128]: the pixels of the grid's cells"""
    a = np.asarray(a).astype(np.int64)
    assert x0 >= 0 and y0 >= 0 and ncx >= 1 and ncy >= 1 and x0 + CELL * ncx <= a.shape[1] and y0 + CELL * ncy <= a.shape[0]
    return a[y0:y0 + CELL * ncy, x0:x0 + CELL * ncx].reshape(ncy, CELL, ncx, CELL)


def records(p, m, x0, y0, ncx, ncy):
    """p, m: u8 [H, W] -> uint32 [ncy, ncx, 6]: sum p, sum p^2, sum p m, sum |p - m|, pixels with p == 0, with p == 255"""
    p, m = _cells(p, x0, y0, ncx, ncy), _cells(m, x0, y0, ncx, ncy)
    parts = [p, p * p, p * m, np.abs(p - m), p == 0, p == 255]
    out = np.stack([q.sum(axis=(1, 3), dtype=np.int64) for q in parts], axis=-1)
    assert out.max() <= N * 255 * 255 < 2 ** 31
    return out.astype(np.uint32)


def model_records(mu, sigma6, x0, y0, ncx, ncy):
    """mu, sigma6: u8 [H, W] -> uint32 [ncy, ncx, 3]: sum m, sum m^2, sum sigma6"""
    m, s = _cells(mu, x0, y0, ncx, ncy), _cells(sigma6, x0, y0, ncx, ncy)
    return np.stack([q.sum(axis=(1, 3), dtype=np.int64) for q in (m, m * m, s)], axis=-1).astype(np.uint32)


def sigma6_of(sigma):
    return np.minimum(6 * np.asarray(sigma).astype(np.int64), 255).astype(np.uint8)


def rdiv(a, b):
    """a / b rounded to the nearest integer, a half upward (Python's // floors toward minus infinity)"""
    assert b > 0
    return (2 * a + b) // (2 * b)


def cell(rec, model):
    """-> dict(rated, clipped, changed, up, ratio)"""
    sp, n_zero, n_sat = int(rec[0]), int(rec[4]), int(rec[5])
    sm, ss6 = int(model[0]), int(model[2])
    lit = sm >= N
    rated = lit and n_zero + n_sat <= N // 16
    changed = rated and abs(sp - sm) > ss6
    return dict(rated=rated, clipped=lit and not rated, changed=changed, up=changed and sp > sm, ratio=rdiv(1000 * sp, sm) if rated else None)


def summary(rec, model):
    """rec [ncy, ncx, 6], model [ncy, ncx, 3] -> dict(rated, clipped, changed, up, down, level_milli, ratio_min, ratio_max,
    gain_milli, offset_milli (None: `-`), kind, changed_cells: bool [ncy, ncx])"""
    rec, model = np.asarray(rec), np.asarray(model)
    shape = rec.shape[:-1]
    cells = [cell(r, m) for r, m in zip(rec.reshape(-1, 6), model.reshape(-1, 3))]
    on = [k for k, c in enumerate(cells) if c["rated"]]
    out = dict(rated=len(on), clipped=sum(c["clipped"] for c in cells), changed=sum(c["changed"] for c in cells),
               up=sum(c["up"] for c in cells), level_milli=None, ratio_min=None, ratio_max=None, gain_milli=None, offset_milli=None,
               changed_cells=np.array([c["changed"] for c in cells], bool).reshape(shape))
    out["down"] = out["changed"] - out["up"]
    if not on:
        out["kind"] = "blind"
        return out
    S = lambda a, w: sum(int(a.reshape(-1, a.shape[-1])[k][w]) for k in on)  # noqa: E731
    Ssp, Sspm, Ssm, Ssmm = S(rec, 0), S(rec, 2), S(model, 0), S(model, 1)
    n = N * len(on)
    out["level_milli"] = rdiv(1000 * (Ssp - Ssm), n)
    out["ratio_min"], out["ratio_max"] = min(cells[k]["ratio"] for k in on), max(cells[k]["ratio"] for k in on)
    var, cov = n * Ssmm - Ssm * Ssm, n * Sspm - Ssp * Ssm
    if var > 0:
        out["gain_milli"] = rdiv(1000 * cov, var)
        out["offset_milli"] = rdiv(1000 * Ssp - out["gain_milli"] * Ssm, n)
    if out["changed"] == 0:
        out["kind"] = "steady"
    elif out["changed"] == len(on) and (out["up"] == 0 or out["down"] == 0):
        out["kind"] = "level"
    else:
        out["kind"] = "uneven"
    return out


def model_arrays(models, W, H, R):
    """-> {cam: uint32 [ncy, ncx, 3]} for every camera with a model (dict(mu=, sigma=))"""
    ncx, ncy, x0, y0 = grid(W, H, R)
    return {c: model_records(m["mu"], sigma6_of(m["sigma"]), x0, y0, ncx, ncy) for c, m in enumerate(models) if m is not None}


def rows_of(stacks, W, H, models, R):
    """stacks: [(event, cam, [(name, image or None or "missing")])] as surveyref.rows_of takes them; models[cam]: None or
    dict(mu=, sigma=) -> light.txt's rows: dicts with event, cam, frame, name, state and rec (None: no record)"""
    ncx, ncy, x0, y0 = grid(W, H, R)
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
                if models[cam] is not None:
                    row["rec"] = records(img, models[cam]["mu"], x0, y0, ncx, ncy)
            rows.append(row)
    return rows


def arrays(models, rows, W, H, R):
    """-> {cam: int32 [N_c, ncy, ncx, 6]} for every camera with a model: what cam<c>_light.npy holds"""
    ncx, ncy, _, _ = grid(W, H, R)
    out = {}
    for c, m in enumerate(models):
        if m is not None:
            mine = [r["rec"] for r in rows if r["cam"] == c and r["rec"] is not None]
            out[c] = np.array(mine, np.int64).astype(np.int32).reshape(len(mine), ncy, ncx, 6)
    return out


def report(models, rows, W, H, R):
    ncx, ncy, x0, y0 = grid(W, H, R) if W > 0 else (0, 0, 0, 0)
    text = f"# abub3hs light 1\nradius {R} cell {CELL} grid {ncx} {ncy} origin {x0} {y0}\n" + HEADER
    mrec = model_arrays(models, W, H, R)
    index = [0] * len(models)
    per_cam = [dict(frames=0, first="-", changed=np.zeros((ncy, ncx), np.int64), **{k: 0 for k in KINDS}) for _ in models]
    dash = lambda v: "-" if v is None else str(v)  # noqa: E731
    for r in rows:
        text += f"{r['event']}\t{r['cam']}\t{r['frame']}\t{r['name']}\t{r['state']}"
        if r["rec"] is None:
            text += "\t-" * 12 + "\n"
            continue
        s, c = summary(r["rec"], mrec[r["cam"]]), per_cam[r["cam"]]
        text += f"\t{index[r['cam']]}" + "".join(f"\t{s[k]}" for k in ("rated", "clipped", "changed", "up", "down"))
        index[r["cam"]] += 1
        text += "".join("\t" + dash(s[k]) for k in ("level_milli", "ratio_min", "ratio_max", "gain_milli", "offset_milli"))
        text += f"\t{s['kind']}\n"
        c["frames"] += 1
        c[s["kind"]] += 1
        c["changed"] += s["changed_cells"]
        if s["changed"] and c["first"] == "-":
            c["first"] = r["event"]
    for c, m in enumerate(models):
        if m is None:
            text += f"light cam {c} none\n"
        else:
            k = per_cam[c]
            text += f"light cam {c} frames {k['frames']} " + " ".join(f"{q} {k[q]}" for q in KINDS) + f" first_changed_event {k['first']}\n"
    for c, m in enumerate(models):
        if m is not None:
            for y in range(ncy):
                text += f"changed cam {c} y {y}" + "".join(f" {int(v)}" for v in per_cam[c]["changed"][y]) + "\n"
    total = {q: sum(per_cam[c][q] for c, m in enumerate(models) if m is not None) for q in ("frames",) + KINDS}
    return text + f"run frames {total['frames']} " + " ".join(f"{q} {total[q]}" for q in KINDS) + "\n"
