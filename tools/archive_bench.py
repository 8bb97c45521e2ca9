#!/usr/bin/env python3
"""abub_zip_pack_dev and abub3hs --repack / --unpack --archive measured on one GPU box -> profiles/r19/archive.json.  Nothing
here is a threshold: the figures are recorded.
  (a) kernel: abub_zip_pack_dev on 1024 resident packed files of 1280x1024 synth frames (the files abub_abf_encode_dev left
      in device memory, each an entry named like a frame of a run), five times after a warm-up, device events, medians; the
      floor of one read plus one write of those bytes at the copy ceilings of DESIGN section 6; and abub_crc32_dev over the
      same files, the unfused comparison (a CRC pass alone, the copy still to come);
  (b) end to end: the 96-event archive of tools/ingest_bench.py (a stored PNG zip); `abub3hs -z --repack DIR [--repack-gpu]
      --archive` of this tree against the directory route of the parent build (--parent), both routes, three alternating
      repetitions, medians of the wall time and of the legs the device route prints (copy back and write split out); the
      host route's archive and the device route's are compared byte for byte once;
  (c) nothing else moved: bench.py --steps 20 --warmup 5, the parent build and this tree alternating, three pairs
      (tools/abf_bench.py part_c); --balanced ORDER: in the balanced order of profiles/r10 instead (tools/verify_bench.py).
usage: python3 tools/archive_bench.py [--parts abc] --parent PARENT_CHECKOUT [--balanced [ORDER]] [--out profiles/r19/archive.json]
       [--frames 1024] [--events 96]"""
import argparse, io, json, os, re, shutil, statistics, subprocess, sys, tempfile, time, zipfile, zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

READ_CEILING_TBPS, FILL_CEILING_TBPS = 6.14, 5.95  # DESIGN section 6 (profiles/r03/copy_ceiling.jsonl)


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def extra_len(off, name_len, length):
    p = -(off + 30 + name_len) % 16
    return 0 if length == 0 or p == 0 else p if p >= 4 else p + 16


def part_a(n, W=1280, H=1024, F=41):
    import torch
    from autobub3hs_amd import _lib, hip, synth
    dev, P = torch.device("cuda:0"), W * H
    fr = np.asarray(synth.render_event(W, H, synth.random_spec(W, H, F, 3, 0), 3, 0))
    frames = torch.from_numpy(fr).to(dev)[torch.arange(n, device=dev) % F].contiguous().reshape(-1)
    files, total, buf = hip.abf_encode(frames, np.arange(n, dtype=np.int64) * P, W, H)
    assert (files[:, 2] == 0).all()
    del frames
    names, rows, off = bytearray(), [], 0
    for k in range(n):
        name = f"20200925_0/{k // 82}/Images/cam{k // 41 % 2}_image{30 + k % 41}.png".encode()
        xl = extra_len(off, len(name), int(files[k, 1]))
        rows.append((int(files[k, 0]), off, int(files[k, 1]), len(names), len(name), xl))
        names += name
        off += 30 + len(name) + xl + int(files[k, 1])
    seg = torch.empty(off + 16, dtype=torch.uint8, device=dev)
    d_names = torch.frombuffer(bytearray(names), dtype=torch.uint8).to(dev)
    L, stream = _lib.lib(), torch.cuda.current_stream().cuda_stream
    rec = np.zeros(n, dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("len", "<u4"), ("name", "<u4"), ("name_len", "<u2"),
                                      ("extra_len", "<u2"), ("reserved", "<u4")]))
    for j, col in enumerate(("src", "dst", "len", "name", "name_len", "extra_len")):
        rec[col] = [r[j] for r in rows]
    d_items = torch.from_numpy(rec.view(np.int64).copy()).to(dev)
    crc = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.full((n,), 99, dtype=torch.int32, device=dev)
    ent = np.zeros((n, 6), dtype=np.uint32)
    ent[:, 2] = files[:, 1]
    ent[:, 4] = files[:, 0] & 0xFFFFFFFF
    ent[:, 5] = files[:, 0] >> 32
    d_ent = torch.from_numpy(ent.view(np.int32).copy()).to(dev)
    crc2 = torch.zeros(n, dtype=torch.int32, device=dev)
    status2 = torch.full((n,), 99, dtype=torch.int32, device=dev)

    def pack():
        _lib.check(L.abub_zip_pack_dev(buf.data_ptr(), total, d_items.data_ptr(), n, d_names.data_ptr(), d_names.numel(), seg.data_ptr(),
                                       off, crc.data_ptr(), status.data_ptr(), stream), "abub_zip_pack_dev")

    def crc_only():
        _lib.check(L.abub_crc32_dev(buf.data_ptr(), buf.numel(), d_ent.data_ptr(), n, crc2.data_ptr(), status2.data_ptr(), stream),
                   "abub_crc32_dev")

    pack()
    crc_only()
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and (status2.cpu().numpy() == 0).all()
    assert torch.equal(crc, crc2)
    for k in (0, n // 3, n - 1):  # (an entry whole: header, name, padding, data)
        src, dst, ln, nm, nl, xl = rows[k]
        data = buf[src:src + ln].cpu().numpy().tobytes()
        got = seg[dst:dst + 30 + nl + xl + ln].cpu().numpy().tobytes()
        assert got[30 + nl + xl:] == data and int.from_bytes(got[14:18], "little") == zlib.crc32(data), k
    t_pack, t_crc = [], []
    for _ in range(5):
        t_pack.append(timed(pack))
        t_crc.append(timed(crc_only))
    ms, ms_crc = statistics.median(t_pack), statistics.median(t_crc)
    floor = (total / READ_CEILING_TBPS + off / FILL_CEILING_TBPS) / 1e9
    return {"files": n, "W": W, "H": H, "file_bytes": int(total), "segment_bytes": int(off), "tile_bytes": 65536,
            "zip_pack_ms": t_pack, "crc32_dev_ms": t_crc, "zip_pack_ms_median": ms, "crc32_dev_ms_median": ms_crc,
            "zip_pack_TBps_read_plus_written": (total + off) / ms / 1e9, "floor_ms_one_read_one_write": floor,
            "times_above_floor": ms / floor, "zip_pack_over_crc32_dev": ms / ms_crc}


def write_archive(tmp, E, W=1280, H=1024, F=41, C=2, run_id="20200925_0"):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from autobub3hs_amd import synth

    def enc(job):
        e, c = job
        st = synth.render_event(W, H, synth.random_spec(W, H, F, e, c, p_second=0.2), e, c)
        out = []
        for k in range(F):
            b = io.BytesIO()
            Image.fromarray(st[k]).save(b, format="PNG", compress_level=1)
            out.append((e, c, k, b.getvalue()))
        return out

    with ThreadPoolExecutor(min(16, len(os.sched_getaffinity(0)))) as ex:
        blobs = [x for l in ex.map(enc, [(e, c) for e in range(E) for c in range(C)]) for x in l]
    os.makedirs(os.path.join(tmp, "png"))
    with zipfile.ZipFile(os.path.join(tmp, "png", run_id + ".zip"), "w", zipfile.ZIP_STORED) as z:
        for e in range(E):
            z.writestr(f"{run_id}/{e}/", b"")
            z.writestr(f"{run_id}/{e}/Images/", b"")
        for e, c, k, data in blobs:
            z.writestr(f"{run_id}/{e}/Images/cam{c}_image{30 + k}.png", data)
    return run_id, E * C * F


LEGS = re.compile(r"read ([\d.]+) s, upload \+ decode ([\d.]+) s, encode ([\d.]+) s, copy back ([\d.]+) s, write ([\d.]+) s")


def part_b(E, parent):
    tmp = tempfile.mkdtemp(prefix="abub_archive_")
    try:
        run_id, total = write_archive(tmp, E)
        print("archive_bench: source archive written", flush=True)
        env = dict(os.environ, ABUB_NUM_CAMS="2", ABUB_THREADS="16")
        exe = {"tree": os.path.join(ROOT, "autobub3hs_amd", "abub3hs"), "parent": os.path.join(parent, "autobub3hs_amd", "abub3hs")}
        cases = {"archive_host": ("tree", ["--archive"]), "archive_gpu": ("tree", ["--repack-gpu", "--archive"]),
                 "parent_directory_host": ("parent", []), "parent_directory_gpu": ("parent", ["--repack-gpu"])}
        runs = {k: [] for k in cases}
        kept = {}
        for rep in range(3):
            for tag, (who, flags) in cases.items():
                out = os.path.join(tmp, "out_" + tag)
                shutil.rmtree(out, ignore_errors=True)
                t0 = time.perf_counter()
                r = subprocess.run([exe[who], "-z", "-d", os.path.join(tmp, "png"), "-r", run_id, "--repack", out] + flags, env=env,
                                   capture_output=True, text=True, timeout=900)
                dt = time.perf_counter() - t0
                assert r.returncode == 0 and f"{total} frames packed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
                row = {"wall_s": dt, "frames_per_s": total / dt}
                m = LEGS.search(r.stdout)
                if m:
                    row.update(zip(("read_s", "decode_s", "encode_s", "copy_s", "write_s"), map(float, m.groups())))
                m = re.search(r"pack ([\d.]+) s", r.stdout)
                if m:
                    row["pack_s"] = float(m.group(1))
                m = re.search(r"archive .*: (\d+) bytes, (\d+) entries", r.stdout)
                if m:
                    row["archive_bytes"], row["archive_entries"] = int(m.group(1)), int(m.group(2))
                    if rep == 0:  # (its CRC-32, taken in pieces; and that it reads as a zip archive)
                        c = 0
                        with open(os.path.join(out, run_id + ".zip"), "rb") as f:
                            for piece in iter(lambda: f.read(1 << 26), b""):
                                c = zlib.crc32(piece, c)
                        kept[tag] = c
                        with zipfile.ZipFile(os.path.join(out, run_id + ".zip")) as z:
                            names = z.namelist()
                            assert len(names) == row["archive_entries"] and z.read(names[-1])[:4] == b"ABF1"
                else:
                    row["files"] = sum(len(fs) for _, _, fs in os.walk(out))
                shutil.rmtree(out, ignore_errors=True)  # (one copy on disk at a time)
                runs[tag].append(row)
                print(f"archive_bench: {tag} {rep}: {row['frames_per_s']:.0f} frames/s", flush=True)
        files = runs["parent_directory_gpu"][0]["files"]
        med = {t: {k: statistics.median(r[k] for r in rows) for k in rows[0] if k not in ("archive_bytes", "archive_entries", "files")}
               for t, rows in runs.items()}
        return {"events": E, "frames": total, "source": "stored archive of level-1 PNG frames, read with -z", "threads": 16,
                "runs": runs, "median": med, "files_of_the_directory_copy": files,
                "archive_gpu_over_parent_directory_gpu": med["archive_gpu"]["frames_per_s"] / med["parent_directory_gpu"]["frames_per_s"],
                "archive_host_over_parent_directory_host": med["archive_host"]["frames_per_s"] / med["parent_directory_host"]["frames_per_s"],
                "host_and_gpu_archives_identical": kept.get("archive_host") == kept.get("archive_gpu")}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--balanced", nargs="?", const="TPPTTPPTTPPT", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "archive.json"))
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--events", type=int, default=96)
    a = ap.parse_args()
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}  # (a second call adds to the first)

    def save(key, value):
        result[key] = value
        print(json.dumps({key: value}), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:  # (written after every part: a later part that fails loses nothing)
            json.dump(result, f, indent=1)

    if "a" in a.parts:
        save("kernel", part_a(a.frames))
    if "b" in a.parts and a.parent:
        save("end_to_end", part_b(a.events, a.parent))
    if "c" in a.parts and a.parent:
        if a.balanced:
            import verify_bench
            save("parent_comparison_" + a.balanced, verify_bench.part_c_balanced(a.parent, a.balanced))
        else:
            import abf_bench
            save("parent_comparison", abf_bench.part_c(a.parent))
