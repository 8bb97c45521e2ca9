"""The numpy restatement of a survey's per-cell shift field ("Surveying a run for local movement"): the
grid of whole cells, the cells' SAD surfaces of abub_frame_shift_cells_dev / fieldCellsHost, a cell's record and its rating,
a frame's kind, the pairing of the rows with their camera's model, field.txt and the arrays of the .npy files.  Nothing here
calls the code under test."""
import numpy as np

CELL = 128
E_RANGE = 1
HEADER = ("event\tcam\tframe\tname\tstate\tindex\trated\tmoved\tmodal_dx\tmodal_dy\tmodal_n\tdx_min\tdx_max\tdy_min\tdy_max\t"
          "kind\n")
KINDS = ("blind", "still", "rigid", "warped", "local")


def grid(W, H, R):
    """-> (ncx, ncy, x0, y0): only whole cells, centred in the interior [R, W - R) x [R, H - R)"""
    iw, ih = max(W - 2 * R, 0), max(H - 2 * R, 0)
    ncx, ncy = iw // CELL, ih // CELL
    return ncx, ncy, R + (iw - CELL * ncx) // 2, R + (ih - CELL * ncy) // 2


def surfaces(p, m, R):
    """p, m: u8 [H, W] -> uint32 [ncy, ncx, 2R+1, 2R+1]: entry [cy, cx, dy + R, dx + R] is the sum over the cell's 128 x 128
    pixels of |p(x + dx, y + dy) - m(x, y)|"""
    p, m = np.asarray(p, np.uint8).astype(np.int16), np.asarray(m, np.uint8).astype(np.int16)  # (differences fit i16)
    H, W = p.shape
    assert m.shape == (H, W)
    ncx, ncy, x0, y0 = grid(W, H, R)
    out = np.zeros((ncy, ncx, 2 * R + 1, 2 * R + 1), np.uint32)
    inner = np.ascontiguousarray(m[y0:y0 + CELL * ncy, x0:x0 + CELL * ncx])
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d = np.abs(p[y0 + dy:y0 + dy + CELL * ncy, x0 + dx:x0 + dx + CELL * ncx] - inner)
            out[:, :, dy + R, dx + R] = d.reshape(ncy, CELL, ncx, CELL).sum(axis=(1, 3), dtype=np.int64)  # (16384 * 255 < 2^32)
    return out


def crop(a, W, H, R, cx, cy):
    """the (128 + 2R)^2 window of a frame around cell (cx, cy): the cell is the interior of the crop at radius R"""
    _, _, x0, y0 = grid(W, H, R)
    return np.ascontiguousarray(a[y0 + CELL * cy - R:y0 + CELL * (cy + 1) + R, x0 + CELL * cx - R:x0 + CELL * (cx + 1) + R])


def record(sad, R):
    """a cell's surface -> [dx, dy, sad0, sad_best, sad_max]: the smallest entry; among equal ones the smaller dx^2 + dy^2, then
    the smaller dy, then the smaller dx"""
    sad = np.asarray(sad).reshape(2 * R + 1, 2 * R + 1)
    v, _, dy, dx = min((int(sad[dy + R, dx + R]), dx * dx + dy * dy, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1))
    return [dx, dy, int(sad[R, R]), v, int(sad.max())]


def records(sad, R):
    """[ncy, ncx, D, D] -> int32 [ncy, ncx, 5]"""
    ncy, ncx = sad.shape[:2]
    return np.array([[record(sad[cy, cx], R) for cx in range(ncx)] for cy in range(ncy)], np.int32).reshape(ncy, ncx, 5)


def rated(rec):
    """the best displacement explains at least half of the worst mismatch"""
    return int(rec[4]) > 0 and 2 * int(rec[3]) <= int(rec[4])


def summary(rec):
    """int32 [ncy, ncx, 5] -> dict(rated, moved, modal (dx, dy, n) or None, ranges (dx_min, dx_max, dy_min, dy_max) or None,
    kind, moved_cells: bool [ncy, ncx])"""
    cells = [(cy, cx) for cy in range(rec.shape[0]) for cx in range(rec.shape[1]) if rated(rec[cy, cx])]
    at = [(int(rec[c][0]), int(rec[c][1])) for c in cells]
    moved_cells = np.zeros(rec.shape[:2], bool)
    for c, d in zip(cells, at):
        moved_cells[c] = d != (0, 0)
    moved = int(moved_cells.sum())
    if not at:
        return dict(rated=0, moved=0, modal=None, ranges=None, kind="blind", moved_cells=moved_cells)
    n, _, dy, dx = min((-at.count(d), d[0] * d[0] + d[1] * d[1], d[1], d[0]) for d in set(at))
    kind = "still" if moved == 0 else "local" if moved < len(at) else "rigid" if len(set(at)) == 1 else "warped"
    xs, ys = [d[0] for d in at], [d[1] for d in at]
    return dict(rated=len(at), moved=moved, modal=(dx, dy, -n), ranges=(min(xs), max(xs), min(ys), max(ys)), kind=kind,
                moved_cells=moved_cells)


def rows_of(stacks, W, H, models, R):
    """stacks: [(event, cam, [(name, image or None or "missing")])] as surveyref.rows_of takes them; models[cam]: None or
    dict(mu=[H, W] u8, ...) -> field.txt's rows: dicts with event, cam, frame, name, state and rec (None: no surface)"""
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
                    row["rec"] = records(surfaces(img, models[cam]["mu"], R), R)
            rows.append(row)
    return rows


def arrays(models, rows, W, H, R):
    """-> {cam: int32 [N_c, ncy, ncx, 5]} for every camera with a model: what cam<c>_field.npy holds"""
    ncx, ncy, _, _ = grid(W, H, R)
    out = {}
    for c, m in enumerate(models):
        if m is not None:
            mine = [r["rec"] for r in rows if r["cam"] == c and r["rec"] is not None]
            out[c] = np.array(mine, np.int32).reshape(len(mine), ncy, ncx, 5)
    return out


def report(models, rows, W, H, R):
    ncx, ncy, x0, y0 = grid(W, H, R) if W > 0 else (0, 0, 0, 0)
    text = f"# abub3hs field 1\nradius {R} cell {CELL} grid {ncx} {ncy} origin {x0} {y0}\n" + HEADER
    index = [0] * len(models)
    per_cam = [dict(frames=0, first="-", moved=np.zeros((ncy, ncx), np.int64), **{k: 0 for k in KINDS}) for _ in models]
    for r in rows:
        text += f"{r['event']}\t{r['cam']}\t{r['frame']}\t{r['name']}\t{r['state']}"
        if r["rec"] is None:
            text += "\t-" * 11 + "\n"
            continue
        s, c = summary(r["rec"]), per_cam[r["cam"]]
        text += f"\t{index[r['cam']]}\t{s['rated']}\t{s['moved']}"
        index[r["cam"]] += 1
        if s["kind"] == "blind":
            text += "\t-" * 7
        else:
            text += "".join(f"\t{v}" for v in s["modal"] + s["ranges"])
        text += f"\t{s['kind']}\n"
        c["frames"] += 1
        c[s["kind"]] += 1
        c["moved"] += s["moved_cells"]
        if s["moved"] and c["first"] == "-":
            c["first"] = r["event"]
    for c, m in enumerate(models):
        if m is None:
            text += f"field cam {c} none\n"
        else:
            k = per_cam[c]
            text += f"field cam {c} frames {k['frames']} " + " ".join(f"{q} {k[q]}" for q in KINDS) + f" first_moved_event {k['first']}\n"
    for c, m in enumerate(models):
        if m is not None:
            for y in range(ncy):
                text += f"moved cam {c} y {y}" + "".join(f" {int(v)}" for v in per_cam[c]["moved"][y]) + "\n"
    total = {q: sum(per_cam[c][q] for c, m in enumerate(models) if m is not None) for q in ("frames",) + KINDS}
    return text + f"run frames {total['frames']} " + " ".join(f"{q} {total[q]}" for q in KINDS) + "\n"


def load_npy(path):
    return np.load(path)
