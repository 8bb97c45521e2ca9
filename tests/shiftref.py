"""The numpy restatement of a survey's shift search ("Surveying a run for movement"): the SAD surface of
abub_frame_shift_dev / frameShiftHost, the tie rule of shiftBest, the pairing of the rows with their camera's model, and the
shift file's text.  Nothing here calls the code under test."""
import numpy as np

E_RANGE = 1
HEADER = "event\tcam\tframe\tname\tstate\tdx\tdy\tat_edge\tsad0\tsad_best\tgain\n"


def surface(p, m, R):
    """p, m: u8 [H, W] -> [2R+1, 2R+1] of Python-int-exact uint64: entry [dy + R, dx + R] is the sum over the interior
    R <= x < W - R, R <= y < H - R of |p(x + dx, y + dy) - m(x, y)|"""
    p, m = np.asarray(p, np.uint8).astype(np.int64), np.asarray(m, np.uint8).astype(np.int64)
    H, W = p.shape
    assert m.shape == (H, W) and W >= 2 * R + 1 and H >= 2 * R + 1
    inner = m[R:H - R, R:W - R]
    out = np.zeros((2 * R + 1, 2 * R + 1), np.uint64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            out[dy + R, dx + R] = int(np.abs(p[R + dy:H - R + dy, R + dx:W - R + dx] - inner).sum())
    return out


def best(sad, R):
    """the smallest entry; among equal ones the smaller dx^2 + dy^2, then the smaller dy, then the smaller dx
    -> dict(dx, dy, at_edge, sad0, sad_best)"""
    sad = np.asarray(sad).reshape(2 * R + 1, 2 * R + 1)
    v, d2, dy, dx = min((int(sad[dy + R, dx + R]), dx * dx + dy * dy, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1))
    return dict(dx=dx, dy=dy, at_edge=abs(dx) == R or abs(dy) == R, sad0=int(sad[R, R]), sad_best=v)


def displaced(texture, dx, dy, W, H, margin):
    """the W x H window of `texture` (at least H + 2 margin by W + 2 margin) whose pixel (x, y) is the texture's pixel
    (margin + x - dx, margin + y - dy): the window at (0, 0) seen through a camera that moved by (dx, dy), so that
    frame(x + dx, y + dy) == model(x, y)"""
    return np.ascontiguousarray(texture[margin - dy:margin - dy + H, margin - dx:margin - dx + W])


def rows_of(stacks, W, H, models, R):
    """stacks: [(event, cam, [(name, image or None or "missing")])] as surveyref.rows_of takes them; models[cam]: None or
    dict(mu=[H, W] u8, ...) -> the shift file's rows: dicts with event, cam, frame, name, state and best (None: no surface)"""
    rows = []
    for event, cam, frames in stacks:
        for i, (name, img) in enumerate(frames):
            row = dict(event=str(event), cam=cam, frame=i, name=name, best=None)
            if isinstance(img, str):
                row["state"] = "missing"
            elif img is None:
                row["state"] = "undecodable"
            elif img.shape != (H, W):
                row["state"] = "other_size"
            else:
                row["state"] = "ok"
                if models[cam] is not None:
                    row["best"] = best(surface(img, models[cam]["mu"], R), R)
            rows.append(row)
    return rows


def report(models, rows, R):
    text = f"# abub3hs shift 1\nradius {R}\n" + HEADER
    for r in rows:
        text += f"{r['event']}\t{r['cam']}\t{r['frame']}\t{r['name']}\t{r['state']}"
        b = r["best"]
        if b is None:
            text += "\t-" * 6 + "\n"
            continue
        gain = 1.0 - b["sad_best"] / float(b["sad0"]) if b["sad0"] else 0.0
        text += f"\t{b['dx']}\t{b['dy']}\t{int(b['at_edge'])}\t{b['sad0']}\t{b['sad_best']}\t{gain:.6f}\n"
    total = [0, 0, 0]
    for c, m in enumerate(models):
        if m is None:
            text += f"shift cam {c} none\n"
            continue
        mine = [r for r in rows if r["cam"] == c and r["best"] is not None]
        moved = [r for r in mine if (r["best"]["dx"], r["best"]["dy"]) != (0, 0)]
        edge = sum(r["best"]["at_edge"] for r in mine)
        text += (f"shift cam {c} frames {len(mine)} at_zero {len(mine) - len(moved)} shifted {len(moved)} at_edge {edge} "
                 f"max_abs_dx {max([abs(r['best']['dx']) for r in mine], default=0)} "
                 f"max_abs_dy {max([abs(r['best']['dy']) for r in mine], default=0)} "
                 f"first_shifted_event {moved[0]['event'] if moved else '-'}\n")
        total = [total[0] + len(mine), total[1] + len(moved), total[2] + edge]
    return text + f"run frames {total[0]} shifted {total[1]} at_edge {total[2]}\n"
