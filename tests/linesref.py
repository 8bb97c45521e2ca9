"""The numpy restatement of the survey's per-line product ("Surveying a run for torn, repeated and banded
frames"): the records of abub_frame_lines_dev / abub::linesHost, the camera's model, the rule for one line and for a frame
in Python ints, and the text and arrays of the files abub3hs --survey-lines writes.  Nothing here calls the project."""
import numpy as np

ROW_WORDS, COL_WORDS, MODEL_WORDS = 5, 3, 3
SHARE, FACTOR, TORN_RUN, OFF_LINES = 4, 4, 8, 4
KINDS = ("blind", "repeated", "torn", "banded", "striped", "steady")
HEADER = ("event\tcam\tframe\tname\tstate\tindex\trated_rows\toff_rows\tstale_rows\tfirst_stale\tlast_stale\trated_cols\toff_cols\t"
          "first_off_row\tlast_off_row\tfirst_off_col\tlast_off_col\tlevel_milli\tkind\n")


def sigma6_of(sigma):
    return np.minimum(6 * sigma.astype(np.int64), 255).astype(np.uint8)


def records(p, mu, r=None):
    """p, mu, r (or None): u8 [H, W] -> (rows int64 [H, 5], cols int64 [W, 3])"""
    p, mu = p.astype(np.int64), mu.astype(np.int64)
    dev, clip = np.abs(p - mu), (p == 0) | (p == 255)
    rows = np.zeros((p.shape[0], ROW_WORDS), np.int64)
    rows[:, 0], rows[:, 1], rows[:, 2] = p.sum(axis=1), dev.sum(axis=1), clip.sum(axis=1)
    if r is not None:
        r = r.astype(np.int64)
        rows[:, 3], rows[:, 4] = np.abs(p - r).sum(axis=1), (p == r).sum(axis=1)
    cols = np.stack([p.sum(axis=0), dev.sum(axis=0), clip.sum(axis=0)], axis=1)
    return rows, cols


def model_records(mu, sigma6):
    """-> (rows int64 [H, 3], cols int64 [W, 3]): sum mu, sum sigma6, pixels with sigma6 == 0"""
    mu, s = mu.astype(np.int64), sigma6.astype(np.int64)
    return (np.stack([mu.sum(axis=1), s.sum(axis=1), (s == 0).sum(axis=1)], axis=1),
            np.stack([mu.sum(axis=0), s.sum(axis=0), (s == 0).sum(axis=0)], axis=1))


def rated(rec, model, N):
    return SHARE * int(rec[2]) <= N and SHARE * int(model[2]) <= N


def rate(rec, model, N, n, S):
    """one line -> dict(state: unrated / rated / off, num = e^2 N, den = (n T)^2; None for an unrated line)"""
    if not rated(rec, model, N):
        return dict(state="unrated", num=None, den=None)
    e = int(n) * (int(rec[0]) - int(model[0])) - int(S)
    num, den = e * e * int(N), (int(n) * int(model[1])) ** 2
    return dict(state="off" if num > FACTOR * den else "rated", num=num, den=den)


def _direction(rec, model, N):
    on = [k for k in range(len(rec)) if rated(rec[k], model[k], N)]
    S = sum(int(rec[k][0]) - int(model[k][0]) for k in on)
    rates = [rate(rec[k], model[k], N, len(on), S) for k in range(len(rec))]
    return on, S, rates


def summary(rows, cols, model_rows, model_cols, has_ref):
    """-> dict of what lines.txt says of a frame, with row_state / col_state (0 unrated, 1 rated, 2 off, 3 stale) and
    ratio_rows / ratio_cols: the largest num / den over the rated lines as a float (0 where den is 0 or none is rated)"""
    H, W = len(rows), len(cols)
    on, S, rr = _direction(rows, model_rows, W)
    onc, _, rc = _direction(cols, model_cols, H)
    state = lambda rates: np.array([("unrated", "rated", "off").index(r["state"]) for r in rates], np.uint8)  # noqa: E731
    rs, cs = state(rr), state(rc)
    stale = [y for y in on if has_ref and int(rows[y][4]) == W]
    run = longest = 0
    for y in range(H):
        run = run + 1 if y in set(stale) else 0
        longest = max(longest, run)
    rs[stale] = 3
    off_r, off_c = [k for k, r in enumerate(rr) if r["state"] == "off"], [k for k, r in enumerate(rc) if r["state"] == "off"]
    ends = lambda v: (v[0], v[-1]) if v else (None, None)  # noqa: E731
    out = dict(rated_rows=len(on), off_rows=len(off_r), stale_rows=len(stale), rated_cols=len(onc), off_cols=len(off_c),
               level_milli=1000 * S // (len(on) * W) if on else 0, row_state=rs, col_state=cs)
    out["first_stale"], out["last_stale"] = ends(stale)
    out["first_off_row"], out["last_off_row"] = ends(off_r)
    out["first_off_col"], out["last_off_col"] = ends(off_c)
    ratio = lambda rates: max([r["num"] / r["den"] for r in rates if r["den"]], default=0.0)  # noqa: E731
    out["ratio_rows"], out["ratio_cols"] = ratio(rr), ratio(rc)
    if 4 * len(on) < H:
        out["kind"] = "blind"
    elif has_ref and len(stale) == len(on):
        out["kind"] = "repeated"
    elif longest >= TORN_RUN:
        out["kind"] = "torn"
    elif len(off_r) >= OFF_LINES:
        out["kind"] = "banded"
    elif len(off_c) >= OFF_LINES:
        out["kind"] = "striped"
    else:
        out["kind"] = "steady"
    return out


def rows_of(stacks, W, H, models):
    """stacks: [(event, cam, [(name, image or None or "missing")])]; models[cam]: None or dict(mu=, sigma=) -> lines.txt's rows:
    dicts with event, cam, frame, name, state, rows / cols (None: no record) and ref (there is a reference frame).  Frame i of
    a stack is paired with frame max(i - 2, 0) of it: the reference is there if that is another row, ok as well"""
    ok = lambda img: not isinstance(img, str) and img is not None and img.shape == (H, W)  # noqa: E731
    out = []
    for event, cam, frames in stacks:
        for i, (name, img) in enumerate(frames):
            row = dict(event=str(event), cam=cam, frame=i, name=name, rows=None, cols=None, ref=False)
            if isinstance(img, str):
                row["state"] = "missing"
            elif img is None:
                row["state"] = "undecodable"
            elif img.shape != (H, W):
                row["state"] = "other_size"
            else:
                row["state"] = "ok"
                ref = max(i - 2, 0)
                if models[cam] is not None:
                    row["ref"] = ref != i and ok(frames[ref][1])
                    row["rows"], row["cols"] = records(img, models[cam]["mu"], frames[ref][1] if row["ref"] else None)
            out.append(row)
    return out


def model_arrays(models):
    """-> {cam: (int32 [H, 3], int32 [W, 3])} for every camera with a model"""
    return {c: tuple(a.astype(np.int32) for a in model_records(m["mu"], sigma6_of(m["sigma"]))) for c, m in enumerate(models) if m is not None}


def arrays(models, rows, W, H):
    """-> {cam: (int32 [N_c, H, 5], int32 [N_c, W, 3])} for every camera with a model"""
    out = {}
    for c, m in enumerate(models):
        if m is not None:
            mine = [r for r in rows if r["cam"] == c and r["rows"] is not None]
            out[c] = (np.array([r["rows"] for r in mine], np.int64).astype(np.int32).reshape(len(mine), H, ROW_WORDS),
                      np.array([r["cols"] for r in mine], np.int64).astype(np.int32).reshape(len(mine), W, COL_WORDS))
    return out


def report(models, rows, W, H, summaries=None):
    """lines.txt; summaries (a list, may be None) gets (row, summary) of every row with a record"""
    text = f"# abub3hs lines 1\nsize {W} {H}\n" + HEADER
    mrec = model_arrays(models)
    per_cam = [dict(frames=0, first="-", rows=np.zeros(max(H, 0), np.int64), cols=np.zeros(max(W, 0), np.int64), **{k: 0 for k in KINDS})
               for _ in models]
    dash = lambda v: "-" if v is None else str(v)  # noqa: E731
    for r in rows:
        text += f"{r['event']}\t{r['cam']}\t{r['frame']}\t{r['name']}\t{r['state']}"
        if r["rows"] is None:
            text += "\t-" * 14 + "\n"
            continue
        s, c = summary(r["rows"], r["cols"], *mrec[r["cam"]], r["ref"]), per_cam[r["cam"]]
        if summaries is not None:
            summaries.append((r, s))
        text += f"\t{c['frames']}\t{s['rated_rows']}\t{s['off_rows']}\t{s['stale_rows']}\t{dash(s['first_stale'])}\t{dash(s['last_stale'])}"
        text += f"\t{s['rated_cols']}\t{s['off_cols']}" + "".join("\t" + dash(s[k]) for k in ("first_off_row", "last_off_row", "first_off_col",
                                                                                               "last_off_col"))
        text += f"\t{s['level_milli']}\t{s['kind']}\n"
        c["frames"] += 1
        c[s["kind"]] += 1
        c["rows"] += s["row_state"] >= 2
        c["cols"] += s["col_state"] >= 2
        if s["kind"] not in ("steady", "blind") and c["first"] == "-":
            c["first"] = r["event"]
    for c, m in enumerate(models):
        if m is None:
            text += f"lines cam {c} none\n"
        else:
            k = per_cam[c]
            text += f"lines cam {c} frames {k['frames']} " + " ".join(f"{q} {k[q]}" for q in KINDS) + f" first_changed_event {k['first']}\n"
    for c, m in enumerate(models):
        if m is not None:
            for word in ("row", "col"):
                text += "".join(f"changed cam {c} {word} {k} frames {int(v)}\n" for k, v in enumerate(per_cam[c][word + "s"]) if v)
    total = {q: sum(per_cam[c][q] for c, m in enumerate(models) if m is not None) for q in ("frames",) + KINDS}
    return text + f"run frames {total['frames']} " + " ".join(f"{q} {total[q]}" for q in KINDS) + "\n"
