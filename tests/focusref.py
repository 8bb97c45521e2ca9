"""The numpy restatement of a survey's per-cell focus records ("Surveying a run for lost focus"): the five
sums of abub_frame_focus_cells_dev / focusCellsHost, the model's three with the coefficient c(u) and nv, rdiv, what a cell
and a frame say, the pairing of the rows with their camera's model, focus.txt and the arrays of the .npy files.  int64 sums
and Python integers; nothing here calls the code under test.  The grid is the field's (fieldref.grid), restated there."""
import numpy as np

from fieldref import CELL, grid  # noqa: F401

N = CELL * CELL
E_RANGE = 1
HEADER = ("event\tcam\tframe\tname\tstate\tindex\trated\tclipped\tchanged\tsofter\tharder\tkeep_milli\tkeep_min\tkeep_max\t"
          "energy_milli\tkind\n")
KINDS = ("blind", "steady", "soft", "uneven")


def _inside(a, x0, y0, ncx, ncy):
    assert x0 >= 1 and y0 >= 1 and ncx >= 1 and ncy >= 1 and x0 + CELL * ncx + 1 <= a.shape[1] and y0 + CELL * ncy + 1 <= a.shape[0]


def gradients(a):
    """[H, W] -> (gx, gy), int64 [H, W]: the central differences a(x + 1, y) - a(x - 1, y) and a(x, y + 1) - a(x, y - 1); the
    frame's outermost ring, where they do not exist, holds 0 and is never read"""
    a = np.asarray(a).astype(np.int64)
    gx, gy = np.zeros_like(a), np.zeros_like(a)
    gx[:, 1:-1] = a[:, 2:] - a[:, :-2]
    gy[1:-1, :] = a[2:, :] - a[:-2, :]
    return gx, gy


def _cells(a, x0, y0, ncx, ncy):
    """int64 [H, W] -> [ncy, 128, ncx, 128]: the pixels of the grid's cells"""
    return a[y0:y0 + CELL * ncy, x0:x0 + CELL * ncx].reshape(ncy, CELL, ncx, CELL)


def records(p, m, x0, y0, ncx, ncy):
    """p, m: u8 [H, W] -> int32 [ncy, ncx, 5]: sum gx^2, sum gy^2, sum gx hx, sum gy hy, pixels with p == 0 or p == 255"""
    p, m = np.asarray(p), np.asarray(m)
    _inside(p, x0, y0, ncx, ncy)
    (gx, gy), (hx, hy) = gradients(p), gradients(m)
    clip = ((p == 0) | (p == 255)).astype(np.int64)
    parts = [gx * gx, gy * gy, gx * hx, gy * hy, clip]
    out = np.stack([_cells(q, x0, y0, ncx, ncy).sum(axis=(1, 3), dtype=np.int64) for q in parts], axis=-1)
    assert np.abs(out).max() <= N * 255 * 255 < 2 ** 31
    return out.astype(np.int32)


def coefficient(m, xa, ya):
    """the coefficient c(u) of p(u) in G = sum over K of gx hx + gy hy, K the cell whose first pixel is (xa, ya): int64
    [130, 130] over K and its ring of one pixel, entry [1 + y - ya, 1 + x - xa]"""
    hx, hy = gradients(m)
    kx = np.zeros((CELL + 4, CELL + 4), np.int64)  # hx and hy on K, 0 elsewhere, with a margin of two
    ky = np.zeros_like(kx)
    kx[2:-2, 2:-2] = hx[ya:ya + CELL, xa:xa + CELL]
    ky[2:-2, 2:-2] = hy[ya:ya + CELL, xa:xa + CELL]
    # c(u) = hx(u - ex) - hx(u + ex) + hy(u - ey) - hy(u + ey), each only where its argument lies in K
    return kx[1:-1, 0:-2] - kx[1:-1, 2:] + ky[0:-2, 1:-1] - ky[2:, 1:-1]


def model_records(mu, sigma6, x0, y0, ncx, ncy):
    """mu, sigma6: u8 [H, W] -> int64 [ncy, ncx, 3]: mxx = sum hx^2, myy = sum hy^2, nv = sum over the cell and its ring of
    (sigma6 c)^2, in Python integers"""
    mu, sigma6 = np.asarray(mu), np.asarray(sigma6)
    _inside(mu, x0, y0, ncx, ncy)
    hx, hy = gradients(mu)
    out = np.zeros((ncy, ncx, 3), np.int64)
    for cy in range(ncy):
        for cx in range(ncx):
            xa, ya = x0 + CELL * cx, y0 + CELL * cy
            c = coefficient(mu, xa, ya)
            s = sigma6[ya - 1:ya + CELL + 1, xa - 1:xa + CELL + 1].astype(np.int64)
            nv = sum(int(v) * int(v) for v in (s * c).reshape(-1))
            assert nv < 2 ** 63
            out[cy, cx] = [int((hx[ya:ya + CELL, xa:xa + CELL] ** 2).sum()), int((hy[ya:ya + CELL, xa:xa + CELL] ** 2).sum()), nv]
    return out


def sigma6_of(sigma):
    return np.minimum(6 * np.asarray(sigma).astype(np.int64), 255).astype(np.uint8)


def rdiv(a, b):
    """a / b rounded to the nearest integer, a half upward (Python's // floors toward minus infinity)"""
    assert b > 0
    return (2 * a + b) // (2 * b)


def cell(rec, model):
    """-> dict(rated, clipped, changed, softer, keep, energy)"""
    gxx, gyy, gxm, gym, n_clip = (int(v) for v in rec)
    mxx, myy, nv = (int(v) for v in model)
    G, M = gxm + gym, mxx + myy
    clipped = n_clip > N // 16
    rated = not clipped and M * M > nv
    changed = rated and (M - G) * (M - G) > nv
    return dict(rated=rated, clipped=clipped, changed=changed, softer=changed and G < M, keep=rdiv(1000 * G, M) if rated else None,
                energy=rdiv(1000 * (gxx + gyy), M) if rated else None)


def summary(rec, model):
    """rec [ncy, ncx, 5], model [ncy, ncx, 3] -> dict(rated, clipped, changed, softer, harder, keep_milli, keep_min, keep_max,
    energy_milli (None: `-`), kind, changed_cells: bool [ncy, ncx])"""
    rec, model = np.asarray(rec), np.asarray(model)
    shape = rec.shape[:-1]
    rec, model = rec.reshape(-1, 5), model.reshape(-1, 3)
    cells = [cell(r, m) for r, m in zip(rec, model)]
    on = [k for k, c in enumerate(cells) if c["rated"]]
    out = dict(rated=len(on), clipped=sum(c["clipped"] for c in cells), changed=sum(c["changed"] for c in cells),
               softer=sum(c["softer"] for c in cells), keep_milli=None, keep_min=None, keep_max=None, energy_milli=None,
               changed_cells=np.array([c["changed"] for c in cells], bool).reshape(shape))
    out["harder"] = out["changed"] - out["softer"]
    if not on:
        out["kind"] = "blind"
        return out
    SG = sum(int(rec[k][2]) + int(rec[k][3]) for k in on)
    SE = sum(int(rec[k][0]) + int(rec[k][1]) for k in on)
    SM = sum(int(model[k][0]) + int(model[k][1]) for k in on)
    out["keep_milli"], out["energy_milli"] = rdiv(1000 * SG, SM), rdiv(1000 * SE, SM)
    out["keep_min"], out["keep_max"] = min(cells[k]["keep"] for k in on), max(cells[k]["keep"] for k in on)
    if out["changed"] == 0:
        out["kind"] = "steady"
    elif out["changed"] == len(on) and out["harder"] == 0:
        out["kind"] = "soft"
    else:
        out["kind"] = "uneven"
    return out


def model_arrays(models, W, H, R):
    """-> {cam: int64 [ncy, ncx, 3]} for every camera with a model (dict(mu=, sigma=))"""
    ncx, ncy, x0, y0 = grid(W, H, R)
    return {c: model_records(m["mu"], sigma6_of(m["sigma"]), x0, y0, ncx, ncy) for c, m in enumerate(models) if m is not None}


def rows_of(stacks, W, H, models, R):
    """stacks: [(event, cam, [(name, image or None or "missing")])] as surveyref.rows_of takes them; models[cam]: None or
    dict(mu=, sigma=) -> focus.txt's rows: dicts with event, cam, frame, name, state and rec (None: no record)"""
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
    """-> {cam: int32 [N_c, ncy, ncx, 5]} for every camera with a model: what cam<c>_focus.npy holds"""
    ncx, ncy, _, _ = grid(W, H, R)
    out = {}
    for c, m in enumerate(models):
        if m is not None:
            mine = [r["rec"] for r in rows if r["cam"] == c and r["rec"] is not None]
            out[c] = np.array(mine, np.int64).astype(np.int32).reshape(len(mine), ncy, ncx, 5)
    return out


def report(models, rows, W, H, R):
    ncx, ncy, x0, y0 = grid(W, H, R) if W > 0 else (0, 0, 0, 0)
    text = f"# abub3hs focus 1\nradius {R} cell {CELL} grid {ncx} {ncy} origin {x0} {y0}\n" + HEADER
    mrec = model_arrays(models, W, H, R)
    index = [0] * len(models)
    per_cam = [dict(frames=0, first="-", changed=np.zeros((ncy, ncx), np.int64), **{k: 0 for k in KINDS}) for _ in models]
    dash = lambda v: "-" if v is None else str(v)  # noqa: E731
    for r in rows:
        text += f"{r['event']}\t{r['cam']}\t{r['frame']}\t{r['name']}\t{r['state']}"
        if r["rec"] is None:
            text += "\t-" * 11 + "\n"
            continue
        s, c = summary(r["rec"], mrec[r["cam"]]), per_cam[r["cam"]]
        text += f"\t{index[r['cam']]}" + "".join(f"\t{s[k]}" for k in ("rated", "clipped", "changed", "softer", "harder"))
        index[r["cam"]] += 1
        text += "".join("\t" + dash(s[k]) for k in ("keep_milli", "keep_min", "keep_max", "energy_milli"))
        text += f"\t{s['kind']}\n"
        c["frames"] += 1
        c[s["kind"]] += 1
        c["changed"] += s["changed_cells"]
        if s["changed"] and c["first"] == "-":
            c["first"] = r["event"]
    for c, m in enumerate(models):
        if m is None:
            text += f"focus cam {c} none\n"
        else:
            k = per_cam[c]
            text += f"focus cam {c} frames {k['frames']} " + " ".join(f"{q} {k[q]}" for q in KINDS) + f" first_changed_event {k['first']}\n"
    for c, m in enumerate(models):
        if m is not None:
            for y in range(ncy):
                text += f"changed cam {c} y {y}" + "".join(f" {int(v)}" for v in per_cam[c]["changed"][y]) + "\n"
    total = {q: sum(per_cam[c][q] for c, m in enumerate(models) if m is not None) for q in ("frames",) + KINDS}
    return text + f"run frames {total['frames']} " + " ".join(f"{q} {total[q]}" for q in KINDS) + "\n"


def blur(img):
    """one pass of the 3 x 3 binomial (1 2 1; 2 4 2; 1 2 1), (sum + 8) / 16, the frame's outermost ring kept"""
    a = np.asarray(img).astype(np.int64)
    out = a.copy()
    s = (a[:-2, :-2] + 2 * a[:-2, 1:-1] + a[:-2, 2:] + 2 * a[1:-1, :-2] + 4 * a[1:-1, 1:-1] + 2 * a[1:-1, 2:] + a[2:, :-2] + 2 * a[2:, 1:-1]
         + a[2:, 2:])
    out[1:-1, 1:-1] = (s + 8) // 16
    return out.astype(np.uint8)
