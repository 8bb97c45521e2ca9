#!/usr/bin/env python3
"""abub_frame_lines_dev and abub3hs --survey --survey-lines [--survey-gpu] measured on one GPU box, in one call ->
profiles/r29/lines.json.  Set and protocol are those of tools/noise_bench.py (its frames, its model, device events, windows
alternating in one call).
  (a) kernel: 1024 resident 1280x1024 synth frames in 25 stacks with a model, every frame against the frame two before it in
      its stack (the second against the first, the first without a reference); three launches per window, five windows alternating with
      abub_frame_noise_cells_dev on the same frames and pairs; ms per launch (median and range), frames per second and the
      bytes moved per second.  The noise kernel reads only the grid's cells, this one whole frames, so the two are compared
      per byte: p and r are frame bytes (W H per frame and stream), mu and sigma6 one plane that every frame reads again,
      most likely from a cache, so each rate is given with and without the plane; some records are checked against
      linesHost first;
  (c) end to end: the 1025-frame run of survey_bench part (c), as PNG files and repacked, surveyed by the CLI on the host
      route and with --survey-gpu, with --survey-lines and without, each three times alternating, from the page cache;
      medians of the CLI's own seconds; the lines' files and the reports compared byte for byte; the kinds lines.txt gives
      this run (all, after the first two frames of each stack, and before and from the frame at which the stack's rendered
      bubble appears) and the largest rule value e^2 N / (n T)^2 over the rows and over the columns, of the frames before
      the bubble and of those with it, from the .npy files;
  (d) parent comparison: bench.py --steps 20 --warmup 5, parent build and this tree in the balanced twelve-run order of
      tools/verify_bench.py, dumped outputs compared byte for byte;
  (t) no GPU: the text of every kernel symbol of this tree's library against the parent build's (llvm-objdump -d, addresses
      stripped): which are equal, which differ, which are new.
usage: python3 tools/lines_bench.py [--parts acdt] [--parent PARENT_CHECKOUT] [--balanced [ORDER]] [--out profiles/r29/lines.json]
                                    [--frames 1024]"""
import argparse, io, json, os, re, shutil, statistics, struct, subprocess, sys, tempfile, time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from survey_bench import F, H, P, W, model_of, part_d, stacks  # noqa: E402

R = 4


def part_a(n):
    import torch
    from autobub3hs_amd import _lib, hip, host

    fr = stacks(n)
    mu, _, s6 = model_of(fr)
    dev = torch.device("cuda:0")
    slab = torch.empty((n, P), dtype=torch.uint8, device=dev)
    for i, (_, _, f) in enumerate(fr):
        slab[i] = torch.from_numpy(f.reshape(-1)).to(dev)
    slab = slab.reshape(-1)
    d_mu = torch.from_numpy(mu.reshape(-1)).to(dev)
    d_s6 = torch.from_numpy(s6.reshape(-1)).to(dev)
    ref = [i - min(fr[i][1], 2) if fr[i][1] else None for i in range(n)]  # (the survey's pairing: frame 0 of a stack has none)
    noise_ref = [i - 2 if fr[i][1] >= 2 else i - fr[i][1] for i in range(n)]  # (tools/noise_bench.py's pairs)
    lines = np.array([[i * P, hip.STAT_NONE if ref[i] is None else ref[i] * P, 0] for i in range(n)], dtype=np.uint64)
    pairs = np.array([[i * P, noise_ref[i] * P, 0] for i in range(n)], dtype=np.int64)
    ncx, ncy, x0, y0 = hip.field_grid(W, H, R)
    cells = ncx * ncy
    status, rows, cols = hip.frame_lines(slab, d_mu, lines, W, H)
    assert not status.any()
    for i in (0, 1, F - 1, n - 1):
        hr, hc = host.lines_host(fr[i][2], mu, None if ref[i] is None else fr[ref[i]][2])
        assert np.array_equal(rows[i], hr) and np.array_equal(cols[i], hc), i
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    d_lines, d_pairs = torch.from_numpy(lines.view(np.int64)).to(dev), torch.from_numpy(pairs).to(dev)
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    out = torch.empty((n * max(cells * 6, H * 5 + W * 3),), dtype=torch.int32, device=dev)

    def lines_k(rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_lines_dev(slab.data_ptr(), slab.numel(), d_mu.data_ptr(), d_mu.numel(), d_lines.data_ptr(), n, W, H,
                                              status.data_ptr(), out.data_ptr(), out.data_ptr() + 4 * n * H * 5, stream), "lines")

    def noise(rep):
        for _ in range(rep):
            _lib.check(L.abub_frame_noise_cells_dev(slab.data_ptr(), slab.numel(), d_s6.data_ptr(), d_s6.numel(), d_pairs.data_ptr(), n, W,
                                                    H, x0, y0, ncx, ncy, status.data_ptr(), out.data_ptr(), stream), "noise")

    def timed(fn, rep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(rep)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / rep

    kernels = {"lines": lines_k, "noise": noise}
    for fn in kernels.values():
        fn(1)
    torch.cuda.synchronize()
    t = {k: [] for k in kernels}
    for _ in range(5):
        for k, fn in kernels.items():
            t[k].append(timed(fn, 3))
    med = {k: statistics.median(v) for k, v in t.items()}
    with_ref = sum(r is not None for r in ref)
    frame_bytes = (n + with_ref) * P  # p of every frame, r of those that have one
    cell_bytes = 2 * n * cells * 16384
    gbs = lambda b, ms: b / ms * 1e3 / 1e9  # noqa: E731
    rates = {"lines_GB_per_s": {"p_and_r": gbs(frame_bytes, med["lines"]), "p_r_and_mu": gbs(frame_bytes + n * P, med["lines"])},
             "noise_GB_per_s": {"p_and_r": gbs(cell_bytes, med["noise"]), "p_r_and_sigma6": gbs(cell_bytes * 3 // 2, med["noise"])}}
    return {"frames": n, "W": W, "H": H, "frames_with_a_reference": with_ref, "noise_grid": [ncx, ncy, x0, y0], "launches_per_window": 3,
            "windows": 5, "ms_per_launch": t, "ms_per_launch_median": med, "ms_per_launch_range": {k: [min(v), max(v)] for k, v in t.items()},
            "frames_per_s": n / med["lines"] * 1e3, "lines_over_noise_time": med["lines"] / med["noise"],
            "frame_bytes_read": {"lines": frame_bytes, "noise": cell_bytes}, **rates,
            "lines_over_noise_rate_per_frame_byte": rates["lines_GB_per_s"]["p_and_r"] / rates["noise_GB_per_s"]["p_and_r"],
            "rate_note": "p and r are frame bytes (r is the p of another job of the same launch); mu and sigma6 are one plane read again "
                         "by every frame, most likely from a cache: only the frame bytes can be set against an HBM read ceiling"}


def lines_summary(d, t0, cam=0):
    """lines.txt and the .npy files of a run of which every frame has a record; t0[event]: the frame at which the event's
    rendered bubble appears.  The kinds of all rows, of the rows after the first two frames of a stack, and of the rows
    before and from their event's bubble on; the largest rule value e^2 N / (n T)^2 over the rated rows and over the rated
    columns (float64), of the frames before the bubble and of the frames with it"""
    text = open(os.path.join(d, "lines.txt")).read()
    rows = [l.split("\t") for l in text.splitlines()[3:] if "\t" in l]
    made = [r for r in rows if r[5] != "-"]
    assert len(made) == len(rows) and [int(r[5]) for r in made] == list(range(len(made)))
    quiet = np.array([int(r[2]) < t0[r[0]] for r in made])

    def count(sel):
        kinds = {}
        for r in made:
            if sel(r):
                kinds[r[18]] = kinds.get(r[18], 0) + 1
        return kinds

    load = lambda s: np.load(os.path.join(d, f"cam{cam}_lines_{s}.npy")).astype(np.int64)  # noqa: E731

    def largest(rec, model, N, frames):
        rec = rec[frames]
        rated = (4 * rec[:, :, 2] <= N) & (4 * model[None, :, 2] <= N)
        D = (rec[:, :, 0] - model[None, :, 0]) * rated
        n = rated.sum(axis=1, keepdims=True)
        e = (n * D - D.sum(axis=1, keepdims=True)).astype(np.float64)
        den = (n * model[None, :, 1]).astype(np.float64) ** 2
        ratio = np.where(rated & (den > 0), e * e * N / np.maximum(den, 1), 0.0)
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        return {"value": float(ratio.max()), "frame": int(np.flatnonzero(frames)[at[0]]), "line": int(at[1])}

    rr, rc, mr, mc = load("rows"), load("cols"), load("model_rows"), load("model_cols")
    values = {part: {"rows": largest(rr, mr, rc.shape[1], sel), "cols": largest(rc, mc, rr.shape[1], sel)}
              for part, sel in (("before_the_bubble", quiet), ("with_the_bubble", ~quiet))}
    return {"rows_with_a_record": len(made), "kinds": count(lambda r: True),
            "kinds_after_the_first_two_frames_of_a_stack": count(lambda r: int(r[2]) >= 2),
            "kinds_before_the_events_bubble": count(lambda r: int(r[2]) < t0[r[0]]),
            "kinds_before_the_events_bubble_after_the_first_two_frames": count(lambda r: 2 <= int(r[2]) < t0[r[0]]),
            "kinds_with_the_events_bubble": count(lambda r: int(r[2]) >= t0[r[0]]),
            "off_rows_before_the_bubble": sum(int(r[7]) for r, q in zip(made, quiet) if q),
            "off_cols_before_the_bubble": sum(int(r[12]) for r, q in zip(made, quiet) if q),
            "stale_rows": sum(int(r[8]) for r in made), "factor": 4, "largest_rule_value": values,
            "level_milli_range": [min(int(r[17]) for r in made), max(int(r[17]) for r in made)],
            "bubble_from_frame": {e: t0[e] for e in sorted(t0, key=int)[:5]},
            "cam_line": [l for l in text.splitlines() if l.startswith("lines cam")]}


def part_c(n):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from autobub3hs_amd import synth

    run_id = "20200925_0"
    exe = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
    env = dict(os.environ, ABUB_NUM_CAMS="1", ABUB_THREADS="16")
    tmp = tempfile.mkdtemp(prefix="abub_lines_")
    # (survey_bench.stacks: stack s is the rendered event s % 5; its bubble is there from the spec's t0 on)
    bubble = {str(s): synth.random_spec(W, H, F, s % 5, 0, p_second=0.2).t0 for s in range((n + F - 1) // F)}
    try:
        n = (n + F - 1) // F * F
        fr = stacks(n)

        def write(job):
            s, k, f = job
            b = io.BytesIO()
            Image.fromarray(f).save(b, format="PNG", compress_level=1)
            os.makedirs(os.path.join(tmp, "png", run_id, str(s), "Images"), exist_ok=True)
            open(os.path.join(tmp, "png", run_id, str(s), "Images", f"cam0_image{30 + k}.png"), "wb").write(b.getvalue())

        with ThreadPoolExecutor(16) as ex:
            list(ex.map(write, fr))
        with open(os.path.join(tmp, "png", run_id, run_id + ".txt"), "w") as f:
            for s in range((n + F - 1) // F):
                f.write(f"{run_id} {s} a b c d e f g h i\n")
        r = subprocess.run([exe, "-d", os.path.join(tmp, "png"), "-r", run_id, "--repack", os.path.join(tmp, "packed"), "--repack-gpu"],
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        out, reports, files, summary = {}, set(), set(), None
        configs = [(route, flag) for flag in (True, False) for route in ("host", "gpu")]
        for kind in ("png", "packed"):
            series = {f"{route}{'_lines' if fl else ''}": [] for route, fl in configs}
            last = {}
            for rep in range(3):
                for route, fl in configs:
                    key = f"{route}{'_lines' if fl else ''}"
                    rep_file, lines_dir = os.path.join(tmp, f"{kind}_{key}.txt"), os.path.join(tmp, f"{kind}_{key}_lines")
                    args = [exe, "-d", os.path.join(tmp, kind), "-r", run_id, "--survey", rep_file]
                    args += ["--survey-lines", lines_dir] if fl else []
                    args += ["--survey-gpu"] if route == "gpu" else []
                    t0 = time.perf_counter()
                    r = subprocess.run(args, env=env, capture_output=True, text=True, timeout=1200)
                    wall = time.perf_counter() - t0
                    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
                    line = [l for l in r.stdout.splitlines() if l.startswith("survey: ")][-1]
                    series[key].append({"survey_s": float(line.rsplit("; ", 1)[1].split(" s,")[0]), "process_s": wall})
                    last[key] = [l.replace(tmp, "TMP") for l in r.stdout.splitlines() if l.startswith("survey")]
                    reports.add(open(rep_file, "rb").read())
                    if fl:
                        d = os.path.join(lines_dir, run_id)
                        files.add(tuple(open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))))
                        if summary is None:
                            summary = lines_summary(d, bubble)
            med = {k: statistics.median(x["survey_s"] for x in v) for k, v in series.items()}
            out[kind] = {"runs": series, "survey_s_median": med, "survey_s_range": {k: [min(x["survey_s"] for x in v), max(x["survey_s"] for x in v)]
                                                                                    for k, v in series.items()},
                         "frames_per_s": {k: n / v for k, v in med.items()},
                         "gpu_over_host_with_lines": med["host_lines"] / med["gpu_lines"], "gpu_over_host_without": med["host"] / med["gpu"],
                         "lines_add_s": {"host": med["host_lines"] - med["host"], "gpu": med["gpu_lines"] - med["gpu"]}, "last_lines": last}
        out["reports_identical"] = len(reports) == 1
        out["lines_files_identical"] = len(files) == 1
        out["frames"] = n
        out["lines_txt_of_this_run"] = summary
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def kernel_texts(lib):
    """{kernel symbol: its instructions' text} of every gfx950 code object inside a built library"""
    data = open(lib, "rb").read()
    texts = {}
    for m in re.finditer(b"\x7fELF\x02\x01\x01\x40", data):
        i = m.start()
        shoff = struct.unpack_from("<Q", data, i + 0x28)[0]
        shentsize, shnum = struct.unpack_from("<HH", data, i + 0x3A)
        with tempfile.NamedTemporaryFile(suffix=".elf", delete=False) as f:
            f.write(data[i:i + shoff + shentsize * shnum])
        dis = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True).stdout
        os.unlink(f.name)
        sym = None
        for line in dis.splitlines():
            head = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if head:
                sym = head.group(1)
                texts[sym] = []
            elif sym and line.strip():
                texts[sym].append(re.sub(r"\s*//.*$", "", line).strip())
    return {k: "\n".join(v) for k, v in texts.items()}


def part_t(parent):
    tree = kernel_texts(os.path.join(ROOT, "autobub3hs_amd", "libabub_hip.so"))
    par = kernel_texts(os.path.join(parent, "autobub3hs_amd", "libabub_hip.so"))
    return {"kernel_symbols": {"tree": len(tree), "parent": len(par)}, "equal_text": sum(k in par and par[k] == v for k, v in tree.items()),
            "different_text": sorted(k for k, v in tree.items() if k in par and par[k] != v), "only_in_tree": sorted(set(tree) - set(par)),
            "only_in_parent": sorted(set(par) - set(tree))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="acdt")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29", "lines.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--balanced", nargs="?", const="TPPTTPPTTPPT", default="TPPTTPPTTPPT")
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):  # (a call that measures some of the parts keeps the others)
        result = json.load(open(a.out))
    for part, fn in (("a", lambda: part_a(a.frames)), ("c", lambda: part_c(a.frames)), ("d", lambda: part_d(a.parent, a.balanced)),
                     ("t", lambda: part_t(a.parent))):
        key = {"a": "kernel", "c": "end_to_end", "d": "parent_comparison_" + a.balanced, "t": "kernel_text_against_the_parent"}[part]
        if part not in a.parts or (part in "dt" and not a.parent):
            result.setdefault(key, "not measured")
            continue
        result[key] = fn()
        print(json.dumps({key: result[key]}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)
