"""Thin Python mirror of the stateless device-pointer launchers (include/abub_hip.h layer A).

torch is plumbing only: it owns the HBM allocations and the stream the kernels are launched on.
"""
import torch

from . import _lib


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.AbubError("device-pointer launcher called with a CPU tensor (no CPU fallback)")
        if t is not None and not t.is_contiguous():
            raise _lib.AbubError("tensor must be contiguous")


def sigma6(sigma):
    _need_cuda(sigma)
    out = torch.empty_like(sigma)
    _lib.check(_lib.lib().abub_sigma6_dev(_ptr(sigma), _ptr(out), sigma.numel(), _stream()), "abub_sigma6_dev")
    return out


def stack_jobs(nstacks, F, first, count, ref_offset, nmodels, device):
    jobs = torch.empty((nstacks * count, 4), dtype=torch.int32, device=device)
    _lib.check(_lib.lib().abub_fill_stack_jobs_dev(_ptr(jobs), nstacks, F, first, count, ref_offset,
                                                   nmodels, _stream()), "abub_fill_stack_jobs_dev")
    return jobs


def make_jobs(rows, device):
    """rows: iterable of (cur, ref, model, out)."""
    return torch.tensor(list(rows), dtype=torch.int64).to(torch.int32).reshape(-1, 4).to(device)


def diff_hist(frames, sigma6_, jobs, W, H, store=False, rows_per_chunk=0, hist=None, diff=None, chain=None):
    """K2. frames: u8 [..,H,W]; sigma6_: u8 [nmodels,H,W]; jobs: int32 [n,4] -> (hist [n,256] i32, diff|None).
    chain=(chain_len, chain_stride): trigger-only form with the stack-structure hint (abub_diff_hist_chained_dev)."""
    _need_cuda(frames, sigma6_, jobs)
    n = jobs.shape[0]
    if hist is None:
        hist = torch.empty((n, 256), dtype=torch.int32, device=frames.device)
    if store and diff is None:
        diff = torch.empty((n, H, W), dtype=torch.uint8, device=frames.device)
    if chain is not None:
        assert rows_per_chunk == 0
        if store:
            _lib.check(_lib.lib().abub_diff_hist_chained_store_dev(_ptr(frames), _ptr(sigma6_), _ptr(jobs), n, W, H,
                                                                   _ptr(hist), _ptr(diff), int(chain[0]), int(chain[1]),
                                                                   _stream()), "abub_diff_hist_chained_store_dev")
            return hist, diff
        _lib.check(_lib.lib().abub_diff_hist_chained_dev(_ptr(frames), _ptr(sigma6_), _ptr(jobs), n, W, H, _ptr(hist),
                                                         int(chain[0]), int(chain[1]), _stream()),
                   "abub_diff_hist_chained_dev")
        return hist, None
    _lib.check(_lib.lib().abub_diff_hist_dev(_ptr(frames), _ptr(sigma6_), _ptr(jobs), n, W, H, _ptr(hist),
                                             _ptr(diff) if store else None, rows_per_chunk, _stream()),
               "abub_diff_hist_dev")
    return hist, (diff if store else None)


def diff_hist_deferred(frames, sigma6_, jobs, W, H, chain):
    """Trigger-only chained K2 with the row machine left out (abub_diff_hist_chained_deferred_dev): -> (hist [n,256] i32,
    state) where state = (pieces, npieces, incomplete u8 [n]); histograms of jobs with incomplete != 0 are not final
    until diff_hist_pieces() has completed them."""
    _need_cuda(frames, sigma6_, jobs)
    n = jobs.shape[0]
    hist = torch.empty((n, 256), dtype=torch.int32, device=frames.device)
    cap = int(_lib.lib().abub_k2_pieces_cap(n, W, H))
    pieces = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=frames.device)
    npieces = torch.zeros((1,), dtype=torch.int32, device=frames.device)
    incomplete = torch.empty((n,), dtype=torch.uint8, device=frames.device)
    _lib.check(_lib.lib().abub_diff_hist_chained_deferred_dev(_ptr(frames), _ptr(sigma6_), _ptr(jobs), n, W, H, _ptr(hist),
                                                              int(chain[0]), int(chain[1]), _ptr(pieces), cap, _ptr(npieces),
                                                              _ptr(incomplete), _stream()),
               "abub_diff_hist_chained_deferred_dev")
    return hist, (pieces, npieces, incomplete)


def diff_hist_pieces(frames, sigma6_, jobs, W, H, hist, state, want):
    """Completes the jobs with want[job] != 0 (u8 [n]) of a diff_hist_deferred() launch: row machine on their handed-over
    rows, histograms finalised in place."""
    _need_cuda(frames, sigma6_, jobs, want)
    pieces, npieces, _ = state
    _lib.check(_lib.lib().abub_diff_hist_pieces_dev(_ptr(frames), _ptr(sigma6_), _ptr(jobs), jobs.shape[0], W, H, _ptr(hist),
                                                    _ptr(pieces), _ptr(npieces), _ptr(want), _stream()),
               "abub_diff_hist_pieces_dev")
    return hist


def k2_set_option(name, value):
    """Run-time K2 launcher knob ("bound", "chain", "budget", "pf", "chunks", ...); results never depend on them."""
    _lib.check(_lib.lib().abub_k2_set_option(name.encode(), int(value)), "abub_k2_set_option")


def k3_set_option(name, value):
    """Run-time K3 launcher knob ("scan", "list", "budget", "chunks"); results never depend on them."""
    _lib.check(_lib.lib().abub_k3_set_option(name.encode(), int(value)), "abub_k3_set_option")


def bound_counts(stream=None):
    """(row pieces handed over to the row machine, global suspect-list entries) of the last bound-and-verify launch on
    `stream` (default: torch's current stream).  Waits for the stream."""
    import ctypes as C

    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    out = (C.c_uint32 * 2)()
    _lib.check(_lib.lib().abub_bound_counts_dev(st, out), "abub_bound_counts_dev")
    return int(out[0]), int(out[1])


def diff_roi(slab, cur, ref, sigma6_, W, H, roi):
    """ProcessFrame ROI overload on frames `cur`,`ref` (indices, ref >= cur... see header) of one slab."""
    _need_cuda(slab, sigma6_)
    rx, ry, rw, rh = roi
    diff = torch.empty((H, W), dtype=torch.uint8, device=slab.device)
    hist = torch.empty((256,), dtype=torch.int32, device=slab.device)
    P = W * H
    base = slab.data_ptr()
    _lib.check(_lib.lib().abub_diff_roi_dev(base + cur * P, base + ref * P, _ptr(sigma6_), W, H, rx, ry, rw, rh,
                                            _ptr(diff), _ptr(hist), _stream()), "abub_diff_roi_dev")
    return diff, hist


def train(frames, W, H, idx=None):
    _need_cuda(frames, idx)
    N = frames.shape[0] if idx is None else idx.numel()
    mu = torch.empty((H, W), dtype=torch.uint8, device=frames.device)
    sg = torch.empty((H, W), dtype=torch.uint8, device=frames.device)
    _lib.check(_lib.lib().abub_train_dev(_ptr(frames), _ptr(idx), N, W, H, _ptr(mu), _ptr(sg), _stream()),
               "abub_train_dev")
    return mu, sg


def pair_hist(frames, pairs, W, H):
    _need_cuda(frames, pairs)
    n = pairs.shape[0]
    hist = torch.empty((n, 256), dtype=torch.int32, device=frames.device)
    _lib.check(_lib.lib().abub_pair_hist_dev(_ptr(frames), _ptr(pairs), n, W, H, _ptr(hist), _stream()),
               "abub_pair_hist_dev")
    return hist


def posttrig(frames, mu, sigma6_, jobs, W, H, store=True):
    _need_cuda(frames, mu, sigma6_, jobs)
    n = jobs.shape[0]
    hist = torch.empty((n, 256), dtype=torch.int32, device=frames.device)
    img = torch.empty((n, H, W), dtype=torch.uint8, device=frames.device) if store else None
    _lib.check(_lib.lib().abub_posttrig_dev(_ptr(frames), _ptr(mu), _ptr(sigma6_), _ptr(jobs), n, W, H,
                                            _ptr(hist), _ptr(img), _stream()), "abub_posttrig_dev")
    return hist, img


def fg_compact(img, thr, cap):
    """img: u8 [n,H,W]; thr: int32 [n] -> (idx int32 [n,cap], count int32 [n])."""
    _need_cuda(img, thr)
    n, H, W = img.shape
    idx = torch.empty((n, cap), dtype=torch.int32, device=img.device)
    cnt = torch.empty((n,), dtype=torch.int32, device=img.device)
    _lib.check(_lib.lib().abub_fg_compact_dev(_ptr(img), n, W, H, _ptr(thr), _ptr(idx), cap, _ptr(cnt),
                                              _stream()), "abub_fg_compact_dev")
    return idx, cnt



def binarize_thr(hist, tozero, W, H):
    """Device Otsu (abub_binarize_thr_dev): hist [n,256] i32, tozero int32 [n] -> thr int32 [n], bit for bit the host's
    binarizeThresholdFromHist(hist[s], W*H, tozero[s])."""
    _need_cuda(hist, tozero)
    n = tozero.numel()
    thr = torch.empty((n,), dtype=torch.int32, device=hist.device)
    _lib.check(_lib.lib().abub_binarize_thr_dev(_ptr(hist), _ptr(tozero), n, W, H, _ptr(thr), _stream()),
               "abub_binarize_thr_dev")
    return thr


def label_blobs(offsets, idx, val, thr, min_box_area, W, H, cap=None, comp=True, in_cap=None):
    """K4b (abub_label_blobs_dev) on a grouped candidate list: offsets int32 [n+1], idx int32 [>= offsets[n]], val u8,
    thr / min_box_area int32 [n] -> dict of device tensors kept_off [n+1], kept_idx [cap], ncomp [n], nkept_comp [n],
    comp_off [n+1], comp [cap, 6] int32 (first, x0, y0, x1, y1, npix) or None, stats [4] (global-path slots, foreground
    pixels, components, kept components).  cap defaults to the list's length (kept <= candidates)."""
    _need_cuda(offsets, idx, val, thr, min_box_area)
    n = thr.numel()
    dev = idx.device
    in_cap = int(idx.numel()) if in_cap is None else int(in_cap)
    cap = max(in_cap, 1) if cap is None else int(cap)
    L = _lib.lib()
    need = int(L.abub_label_blobs_scratch_bytes(n, W, H, in_cap, 1 if comp else 0))
    scratch = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    out = {"kept_off": torch.empty((n + 1,), dtype=torch.int32, device=dev),
           "kept_idx": torch.empty((cap,), dtype=torch.int32, device=dev),
           "ncomp": torch.empty((n,), dtype=torch.int32, device=dev),
           "nkept_comp": torch.empty((n,), dtype=torch.int32, device=dev),
           "comp_off": torch.empty((n + 1,), dtype=torch.int32, device=dev),
           "comp": torch.empty((cap, 6), dtype=torch.int32, device=dev) if comp else None,
           "stats": torch.empty((4,), dtype=torch.int32, device=dev)}
    _lib.check(L.abub_label_blobs_dev(_ptr(offsets), _ptr(idx), _ptr(val), in_cap, n, W, H, _ptr(thr), _ptr(min_box_area),
                                      _ptr(out["kept_off"]), _ptr(out["kept_idx"]), cap, _ptr(out["ncomp"]),
                                      _ptr(out["nkept_comp"]), _ptr(out["comp_off"]), _ptr(out["comp"]), cap if comp else 0,
                                      _ptr(out["stats"]), _ptr(scratch), scratch.numel(), _stream()),
               "abub_label_blobs_dev")
    return out

def trace_contours_limits():
    """(max_pixels, max_chain) of K5: a slot with more kept pixels, or with a border chain of more codes, is declined."""
    import ctypes as C
    mp, mc = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().abub_trace_contours_limits(C.byref(mp), C.byref(mc)), "abub_trace_contours_limits")
    return mp.value, mc.value


def trace_contours(kept_off, kept_idx, W, H, cont_cap=None, pts_cap=None, in_cap=None):
    """K5 (abub_trace_contours_dev) on K4b's kept lists: kept_off int32 [n+1], kept_idx int32 -> dict of device tensors
    status [n] (0 traced, 1 declined: trace on the host), ncont [n], cont_off [n+1], cont_npts [cont_cap], pt_off [n+1],
    pts [pts_cap] (x | y << 16), stats [4] (slots traced, slots declined, contours, vertices).  Offsets are true counts;
    the capacities default to the list's length and four times it."""
    _need_cuda(kept_off, kept_idx)
    n = kept_off.numel() - 1
    dev = kept_idx.device
    in_cap = int(kept_idx.numel()) if in_cap is None else int(in_cap)
    cont_cap = max(in_cap, 1) if cont_cap is None else int(cont_cap)
    pts_cap = max(4 * in_cap, 1) if pts_cap is None else int(pts_cap)
    L = _lib.lib()
    need = int(L.abub_trace_contours_scratch_bytes(n, in_cap))
    scratch = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    out = {"status": torch.empty((n,), dtype=torch.int32, device=dev),
           "ncont": torch.empty((n,), dtype=torch.int32, device=dev),
           "cont_off": torch.empty((n + 1,), dtype=torch.int32, device=dev),
           "cont_npts": torch.empty((cont_cap,), dtype=torch.int32, device=dev),
           "pt_off": torch.empty((n + 1,), dtype=torch.int32, device=dev),
           "pts": torch.empty((pts_cap,), dtype=torch.int32, device=dev),
           "stats": torch.empty((4,), dtype=torch.int32, device=dev)}
    _lib.check(L.abub_trace_contours_dev(_ptr(kept_off), _ptr(kept_idx), in_cap, n, W, H, _ptr(out["status"]),
                                         _ptr(out["ncont"]), _ptr(out["cont_off"]), _ptr(out["cont_npts"]), cont_cap,
                                         _ptr(out["pt_off"]), _ptr(out["pts"]), pts_cap, _ptr(out["stats"]), _ptr(scratch),
                                         scratch.numel(), _stream()), "abub_trace_contours_dev")
    return out

def trigger_search_limits():
    """(max_frames, max_segs) of K6: a stack with more frames or more segments keeps the host search."""
    import ctypes as C
    mf, ms = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().abub_trigger_search_limits(C.byref(mf), C.byref(ms)), "abub_trigger_search_limits")
    return mf.value, ms.value


TRIG_DONE, TRIG_NEED_FRAMES, TRIG_NEED_FINAL, TRIG_BAD_LOOKAHEAD = 0, 1, 2, 3


def trigger_search(stacks, W, H, sig_main=True):
    """K6 (abub_trigger_search_dev): one trigger search per stack in one launch.  stacks: a list of dicts with F, tss and
    segs = [(first, hist, pending)] (hist: int32 device tensor [count, 256], pending: uint8 device tensor [count] or
    None), optionally start (1) and first_bad (F).  -> (list of result dicts with the fields of abub_trig_result,
    sig_main: float64 tensor [nstacks, max F] filled with NaN where the search evaluated no main-loop frame, or None).
    W * H <= 2^31 - 65 (ABUB_TRIG_MAX_PIXELS), the largest pixel count whose float stays below 2^31: the search converts
    float counts and its float pixel counter to int.  A larger one is refused."""
    import ctypes as C
    import struct
    n = len(stacks)
    nseg = sum(len(s["segs"]) for s in stacks)
    st = (_lib.TrigStack * max(n, 1))()
    sg = (_lib.TrigSeg * max(nseg, 1))()
    k = 0
    dev = None
    for i, s in enumerate(stacks):
        st[i].seg0, st[i].nseg, st[i].F, st[i].tss = k, len(s["segs"]), s["F"], s["tss"]
        st[i].start, st[i].first_bad = s.get("start", 1), s.get("first_bad", s["F"])
        for first, hist, pending in s["segs"]:
            _need_cuda(hist, pending)
            dev = hist.device
            sg[k].hist, sg[k].pending, sg[k].first, sg[k].count = _ptr(hist), _ptr(pending), first, hist.shape[0]
            k += 1
    if dev is None:
        dev = torch.device("cuda")
    L = _lib.lib()
    nbytes = int(L.abub_trigger_search_desc_bytes(n, nseg))
    desc = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
    out = torch.zeros((max(n, 1), 8), dtype=torch.int32, device=dev)
    pitch = max([s["F"] for s in stacks] + [1])
    sm = torch.full((max(n, 1), pitch), float("nan"), dtype=torch.float64, device=dev) if sig_main else None
    _lib.check(L.abub_trigger_search_dev(C.addressof(st), C.addressof(sg), n, nseg, W, H, _ptr(desc), desc.numel(), _ptr(out),
                                         _ptr(sm), pitch, _stream()), "abub_trigger_search_dev")
    rows = out.cpu().numpy()  # (synchronises: the host arrays above stay alive until here)
    names = ("state", "status", "trig", "loc_thres", "need_frame", "evaluated")
    res = []
    for i in range(n):
        r = {k_: int(rows[i, j]) for j, k_ in enumerate(names)}
        r["sig"] = struct.unpack("<f", struct.pack("<i", int(rows[i, 6])))[0]
        res.append(r)
    return res, (sm[:n] if sig_main else None)


# ---- PNG frames decoded on the GPU (abub_png_decode_dev) --------------------------------------------------------
PNG_SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def png_kind(ctype, depth):
    """abub_png_frame.kind of a PNG's colour type and bit depth: 0 for the two 8-bit kinds of abub_png_decode_dev, colour
    type | depth << 8 for the 13 typed kinds of abub_png_decode_typed_dev, None for what no decoder here reads."""
    if depth == 8 and ctype in (0, 3):
        return 0
    ok = {0: (1, 2, 4, 16), 3: (1, 2, 4), 2: (8, 16), 4: (8, 16), 6: (8, 16)}
    return ctype | depth << 8 if depth in ok.get(ctype, ()) else None


PNG_KIND_ADAM7 = 1 << 16  # ABUB_PNG_KIND_ADAM7
_ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))  # x0, y0, dx, dy


def png_adam7_bytes(W, H, bits):
    """Bytes of the inflated stream of an Adam7-interlaced W x H image of `bits` per pixel: the scanlines (filter type + row)
    of the passes that have pixels."""
    n = 0
    for x0, y0, dx, dy in _ADAM7:
        pw, ph = max(0, -(-(W - x0) // dx)), max(0, -(-(H - y0) // dy))
        if pw and ph:
            n += ph * ((pw * bits + 7) // 8 + 1)
    return n


def png_parse(data, W, H, types=False, adam7=False):
    """What the host does per file before the upload: walk the chunks of a PNG, -> (idat segments [(offset, length)],
    palette->grey table (bytes, 256) or None) for an 8-bit grey / 8-bit palette image of W x H without interlace, or None
    for anything the GPU path does not take (the caller decodes such a file on the host).  types=True: the typed walk
    (host.png_walk_typed restated) -> (segments, table or None, kind) for every non-interlaced type the host decoder reads.
    adam7=True (host.png_walk_adam7 restated, types as its `typed`): an Adam7-interlaced file of a kind the walk takes anyway
    is accepted too, -> (segments, table or None, kind) with PNG_KIND_ADAM7 set in the kind of such a file."""
    import struct
    if len(data) < 33 or data[:8] != b"\x89PNG\r\n\x1a\n":
        return None
    o, segs, pal, hdr, end = 8, [], None, None, False
    while not end and o + 12 <= len(data):
        ln, = struct.unpack(">I", data[o:o + 4])
        typ = data[o + 4:o + 8]
        if o + 12 + ln > len(data):
            return None
        if typ == b"IHDR" and ln >= 13:
            hdr = struct.unpack(">IIBBBBB", data[o + 8:o + 21])
        elif typ == b"PLTE":
            pal = data[o + 8:o + 8 + ln]
        elif typ == b"IDAT":
            segs.append((o + 8, ln))
        elif typ == b"IEND":
            end = True
        o += 12 + ln
    if hdr is None or not segs or hdr[0] != W or hdr[1] != H or not (hdr[6] == 0 or (adam7 and hdr[6] == 1)):
        return None
    kind = png_kind(hdr[3], hdr[2])
    if kind is None or (kind != 0 and not types):
        return None
    if hdr[6]:
        if png_adam7_bytes(W, H, PNG_SAMPLES[hdr[3]] * hdr[2]) >= 1 << 31:
            return None
        kind |= PNG_KIND_ADAM7
    elif kind and H * ((W * PNG_SAMPLES[hdr[3]] * hdr[2] + 7) // 8 + 1) >= 1 << 31:
        return None
    lut = None
    if hdr[3] == 3:
        n = min(len(pal or b"") // 3, 256)
        lut = bytes(((pal[3 * i] * 9797 + pal[3 * i + 1] * 19234 + pal[3 * i + 2] * 3737 + 16384) >> 15) & 255 if i < n else 0
                    for i in range(256))
    return (segs, lut, kind) if types or adam7 else (segs, lut)


def png_decode(files, W, H, device="cuda:0", types=False, kinds=None, dsts=None, out=None, out_bytes=None, adam7=False,
               raw_stride=None):
    """files: list of bytes objects (PNG files) -> (frames u8 [n, H, W] on the device, status i32 [n] on the host).  A file
    png_parse() refuses gets status -1 and a frame left untouched (zeros).  types=True: the typed walk and
    abub_png_decode_typed_dev, the raw stride that of the widest kind among the files.  For tests of the descriptor checks
    (types=True): kinds[i] / dsts[i], where not None, replace the kind the walk found / the frame's byte offset in `out`;
    out: a u8 device tensor to decode into instead of a new one (returned as it is), out_bytes: how many of its bytes the
    kernels are told of (what lies behind them must stay as it is).  adam7=True: the walk with adam7 (types as its `typed`)
    and abub_png_decode_adam7_dev, the raw stride the largest abub_png_raw_stride_adam7 among the files -- or raw_stride, for
    tests of the stride check; kinds / dsts as with types=True."""
    import numpy as np
    n = len(files)
    frames_np = np.zeros((max(n, 1), 8), dtype=np.uint32)
    segs, luts, blob, zoff = [], [], bytearray(), 0
    status_pre = np.zeros(n, dtype=np.int32)
    P = W * H
    L = _lib.lib()
    stride = int(L.abub_png_raw_stride(W, H))
    for i, data in enumerate(files):
        parsed = png_parse(data, W, H, types, adam7)
        base = len(blob)
        dst = i * P if dsts is None or dsts[i] is None else int(dsts[i])
        if parsed is None:
            status_pre[i] = -1
            frames_np[i] = (len(segs), 0, zoff, 0, 0xFFFFFFFF, 0, (i * P) & 0xFFFFFFFF, (i * P) >> 32)
            zoff += 16
            continue
        sg, lut = parsed[:2]
        kind = parsed[2] if types or adam7 else 0
        if (types or adam7) and kinds is not None and kinds[i] is not None:
            kind = int(kinds[i])
        if adam7:
            stride = max(stride, int(L.abub_png_raw_stride_adam7(W, H, kind)))
        elif types:
            stride = max(stride, int(L.abub_png_raw_stride_kind(W, H, kind)))
        zlen = sum(l for _, l in sg)
        li = 0xFFFFFFFF
        if lut is not None:
            li = len(luts)
            luts.append(lut)
        frames_np[i] = (len(segs), len(sg), zoff, zlen, li, kind, dst & 0xFFFFFFFF, dst >> 32)
        segs += [(base + o, l) for o, l in sg]
        blob += data
        blob += b"\0" * ((-len(blob)) % 4)
        zoff += ((zlen + 15) & ~15) + 16
    blob += b"\0" * 8
    if adam7 and raw_stride is not None:
        stride = int(raw_stride)
    dev = torch.device(device)
    d_files = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    d_frames = torch.from_numpy(frames_np.view(np.int32).copy()).to(dev)
    d_segs = torch.tensor(segs if segs else [(0, 0)], dtype=torch.int64).to(torch.int32).to(dev) if True else None
    d_luts = torch.frombuffer(bytearray(b"".join(luts) if luts else bytes(256)), dtype=torch.uint8).to(dev)
    d_z = torch.empty((max(zoff, 16),), dtype=torch.uint8, device=dev)
    d_raw = torch.empty((max(n, 1) * stride,), dtype=torch.uint8, device=dev)
    given = out is not None
    if given:
        _need_cuda(out)
    else:
        out = torch.zeros((max(n, 1), H, W), dtype=torch.uint8, device=dev)
    status = torch.full((max(n, 1),), 99, dtype=torch.int32, device=dev)
    nout = out.numel() if out_bytes is None else min(int(out_bytes), out.numel())
    if adam7:
        _lib.check(L.abub_png_decode_adam7_dev(_ptr(d_files), d_files.numel(), _ptr(d_frames), n, _ptr(d_segs), len(segs),
                                               _ptr(d_luts), len(luts), W, H, _ptr(d_z), d_z.numel(), _ptr(d_raw), d_raw.numel(),
                                               stride, _ptr(out), nout, _ptr(status), _stream()),
                   "abub_png_decode_adam7_dev")
    elif types:
        _lib.check(L.abub_png_decode_typed_dev(_ptr(d_files), d_files.numel(), _ptr(d_frames), n, _ptr(d_segs), len(segs),
                                               _ptr(d_luts), len(luts), W, H, _ptr(d_z), d_z.numel(), _ptr(d_raw), d_raw.numel(),
                                               stride, _ptr(out), nout, _ptr(status), _stream()),
                   "abub_png_decode_typed_dev")
    else:
        _lib.check(L.abub_png_decode_dev(_ptr(d_files), d_files.numel(), _ptr(d_frames), n, _ptr(d_segs), len(segs),
                                         _ptr(d_luts), len(luts), W, H, _ptr(d_z), d_z.numel(), _ptr(d_raw), d_raw.numel(),
                                         _ptr(out), nout, _ptr(status), _stream()), "abub_png_decode_dev")
    st = status.cpu().numpy()[:n].copy()
    st[status_pre != 0] = -1
    return (out if given else out[:n]), st


def abf_decode(files, descs, W, H, out, status=None):
    """abub_abf_decode_dev: files u8 [files_bytes] (packed "ABF1" files as they are on disk, anywhere in the buffer), descs
    int64 [n, 3] of (offset of the file, its length, byte offset of its decoded frame in `out`), out u8 (any shape, written
    in place) -> status i32 [n] on the device (0 = decoded, else ABUB_ABF_E_*)."""
    import numpy as np
    _need_cuda(files, out)
    d = np.asarray(descs, dtype=np.int64).reshape(-1, 3)
    n = len(d)
    rec = np.zeros((max(n, 1), 4), dtype=np.uint32)
    rec[:n, 0] = d[:, 0] & 0xFFFFFFFF
    rec[:n, 1] = d[:, 1] & 0xFFFFFFFF
    rec[:n, 2] = d[:, 2] & 0xFFFFFFFF
    rec[:n, 3] = d[:, 2] >> 32
    d_desc = torch.from_numpy(rec.view(np.int32).copy()).to(files.device)
    if status is None:
        status = torch.full((max(n, 1),), 99, dtype=torch.int32, device=files.device)
    _lib.check(_lib.lib().abub_abf_decode_dev(_ptr(files), files.numel(), _ptr(d_desc), n, W, H, _ptr(out), out.numel(),
                                              _ptr(status), _stream()), "abub_abf_decode_dev")
    return status[:n]


# ---- BMP frames decoded on the GPU (abub_bmp_decode_dev) ----------------------------------------------------------
def bmp_parse(data, W, H):
    """What the host does per file before the upload (host/bmpwalk.hpp::bmpWalk restated): the header of a BMP -> dict of
    data_off, stride, bpp, top_down, identity and lut (bytes, 256: index -> grey; the identity for 24 / 32 bit) for a file
    the host decoder (decodeBMP, host/cvlite.cpp) reads as a W x H image, or None for anything else."""
    import struct
    size = len(data)
    if size < 54 or data[:2] != b"BM":
        return None
    data_off, hdr, w, h = struct.unpack_from("<IIii", data, 10)
    bpp, comp = struct.unpack_from("<HI", data, 28)
    ncol, = struct.unpack_from("<I", data, 46)
    if hdr < 40:
        return None
    top_down = h < 0
    h = abs(h)
    if w <= 0 or h <= 0 or (comp != 0 and not (comp == 3 and bpp == 32)) or bpp not in (1, 4, 8, 24, 32):
        return None
    if w != W or h != H:
        return None
    stride = (w * bpp + 31) // 32 * 4
    if data_off + stride * h > size:
        return None
    lut = list(range(256))
    if bpp <= 8:
        if ncol == 0:
            ncol = 1 << bpp
        po = (14 + hdr) & 0xFFFFFFFF
        for i in range(min(ncol, 256)):
            if po + 4 * i + 3 >= size:
                break
            b, g, r = data[po + 4 * i], data[po + 4 * i + 1], data[po + 4 * i + 2]
            lut[i] = ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14) & 255
    return dict(data_off=data_off, stride=stride, bpp=bpp, top_down=top_down, identity=lut == list(range(256)), lut=bytes(lut))


def bmp_decode(files, descs, luts, W, H, out, status=None):
    """abub_bmp_decode_dev: files u8 [files_bytes] (BMP files as they are on disk, anywhere in the buffer), descs: rows of
    (off, len, data_off, stride, bpp, flags, lut, dst) as abub_bmp_frame (lut 0xffffffff: none), luts u8 [nluts * 256] or
    None, out u8 (any shape, written in place) -> status i32 [n] on the device (0 = decoded, else ABUB_BMP_E_DESC)."""
    import numpy as np
    _need_cuda(files, out, luts)
    d = np.asarray(descs, dtype=np.int64).reshape(-1, 8)
    n = len(d)
    rec = np.zeros((max(n, 1), 8), dtype=np.uint32)
    rec[:n, 0:4] = d[:, 0:4] & 0xFFFFFFFF
    rec[:n, 4] = (d[:, 4] & 0xFFFF) | ((d[:, 5] & 0xFFFF) << 16)
    rec[:n, 5] = d[:, 6] & 0xFFFFFFFF
    rec[:n, 6] = d[:, 7] & 0xFFFFFFFF
    rec[:n, 7] = d[:, 7] >> 32
    d_desc = torch.from_numpy(rec.view(np.int32).copy()).to(files.device)
    if status is None:
        status = torch.full((max(n, 1),), 99, dtype=torch.int32, device=files.device)
    nluts = 0 if luts is None else luts.numel() // 256
    _lib.check(_lib.lib().abub_bmp_decode_dev(_ptr(files), files.numel(), _ptr(d_desc), n, _ptr(luts), nluts, W, H, _ptr(out),
                                              out.numel(), _ptr(status), _stream()), "abub_bmp_decode_dev")
    return status[:n]


# ---- deflated zip entries inflated on the GPU (abub_unzip_dev) --------------------------------------------------------
def _zip_entries(entries, device):
    import numpy as np
    d = np.asarray(entries, dtype=np.int64).reshape(-1, 5)
    n = len(d)
    rec = np.zeros((max(n, 1), 6), dtype=np.uint32)
    rec[:n, 0:4] = d[:, 0:4] & 0xFFFFFFFF
    rec[:n, 4] = d[:, 4] & 0xFFFFFFFF
    rec[:n, 5] = d[:, 4] >> 32
    return n, torch.from_numpy(rec.view(np.int32).copy()).to(device)


def unzip(comp, entries, out, status=None):
    """abub_unzip_dev: comp u8 [comp_bytes] (raw deflate streams as they lie in an archive), entries: rows of
    (off, clen, ulen, crc, dst) as abub_zip_entry, out u8 (written in place) -> status i32 [n] on the device (0 = inflated,
    exactly ulen bytes with that CRC-32; else ABUB_ZIP_E_DESC = 1, a deflate status with the number of its ABUB_PNG_E_*, or
    ABUB_ZIP_E_CRC = 16)."""
    _need_cuda(comp, out)
    n, d_ent = _zip_entries(entries, comp.device)
    if status is None:
        status = torch.full((max(n, 1),), 99, dtype=torch.int32, device=comp.device)
    _lib.check(_lib.lib().abub_unzip_dev(_ptr(comp), comp.numel(), _ptr(d_ent), n, _ptr(out), out.numel(), _ptr(status), _stream()),
               "abub_unzip_dev")
    return status[:n]


def crc32(buf, entries):
    """abub_crc32_dev (the CRC kernel of abub_unzip_dev alone): entries as for unzip (only ulen and dst are looked at) ->
    (crc int64 [n] on the host, what zlib.crc32 gives the ulen bytes at buf + dst; status i32 [n] on the host)."""
    _need_cuda(buf)
    n, d_ent = _zip_entries(entries, buf.device)
    crc = torch.zeros((max(n, 1),), dtype=torch.int32, device=buf.device)
    status = torch.full((max(n, 1),), 99, dtype=torch.int32, device=buf.device)
    _lib.check(_lib.lib().abub_crc32_dev(_ptr(buf), buf.numel(), _ptr(d_ent), n, _ptr(crc), _ptr(status), _stream()), "abub_crc32_dev")
    return (crc[:n].cpu().to(torch.int64) & 0xFFFFFFFF), status[:n].cpu()


def zip_pack(buf, items, names, seg, crc=None, status=None, buf_bytes=None, names_bytes=None, seg_bytes=None):
    """abub_zip_pack_dev: buf u8 (resident files), items: rows of (src, dst, len, name, name_len, extra_len) as
    abub_zip_item, names u8 (the entries' names), seg u8 (written in place: per item its local header, name, padding field
    and data at dst, nothing else) -> (crc int64 [n] on the host, what zlib.crc32 gives the len bytes at buf + src;
    status i32 [n] on the host: 0, or ABUB_ZIP_E_DESC = 1 and nothing of the item written).  crc / status: i32 device
    tensors to reuse; *_bytes: what the kernels may touch of a buffer, default all of it."""
    import numpy as np
    _need_cuda(buf, names, seg, crc, status)
    d = np.asarray(items, dtype=np.int64).reshape(-1, 6)
    n = len(d)
    rec = np.zeros((max(n, 1),), dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("len", "<u4"), ("name", "<u4"),
                                                  ("name_len", "<u2"), ("extra_len", "<u2"), ("reserved", "<u4")]))
    for k, col in enumerate(("src", "dst", "len", "name", "name_len", "extra_len")):
        rec[col][:n] = d[:, k].astype(np.uint64)
    d_items = torch.from_numpy(rec.view(np.int64).copy()).to(buf.device)
    if crc is None:
        crc = torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32, device=buf.device)
    if status is None:
        status = torch.full((max(n, 1),), 99, dtype=torch.int32, device=buf.device)
    _lib.check(_lib.lib().abub_zip_pack_dev(_ptr(buf), buf.numel() if buf_bytes is None else int(buf_bytes), _ptr(d_items), n,
                                            _ptr(names), names.numel() if names_bytes is None else int(names_bytes), _ptr(seg),
                                            seg.numel() if seg_bytes is None else int(seg_bytes), _ptr(crc), _ptr(status), _stream()),
               "abub_zip_pack_dev")
    return (crc[:n].cpu().to(torch.int64) & 0xFFFFFFFF), status[:n].cpu()


def _encode(entry_name, bound_name, scratch_name, pixels, src, W, H, out, scratch, out_cap):
    """one call of an encoder's entry: what abf_encode and png_encode share (their arguments and results)"""
    import numpy as np
    _need_cuda(pixels, out, scratch)
    L = _lib.lib()
    offs = np.asarray(src, dtype=np.int64).reshape(-1)
    n = len(offs)
    dev = pixels.device
    d_src = torch.from_numpy(np.concatenate([offs, np.zeros(1, np.int64)])).to(dev)
    if out is None:
        out = torch.empty((max(n, 1) * ((int(getattr(L, bound_name)(W, H)) + 15) & ~15),), dtype=torch.uint8, device=dev)
    need = int(getattr(L, scratch_name)(n, W, H))
    if scratch is None:
        scratch = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    d_files = torch.zeros((max(n, 1), 2), dtype=torch.int64, device=dev)
    d_total = torch.zeros((1,), dtype=torch.int64, device=dev)
    cap = out.numel() if out_cap is None else min(int(out_cap), out.numel())
    _lib.check(getattr(L, entry_name)(_ptr(pixels), pixels.numel(), _ptr(d_src), n, W, H, _ptr(out), cap, _ptr(d_files), _ptr(d_total),
                                      _ptr(scratch), scratch.numel(), _stream()), entry_name)
    rec = d_files.cpu().numpy()[:n]
    files = np.stack([rec[:, 0], rec[:, 1] & 0xFFFFFFFF, rec[:, 1] >> 32], axis=1) if n else np.zeros((0, 3), np.int64)
    return files, int(d_total.item()), out


def abf_encode(pixels, src, W, H, out=None, scratch=None, out_cap=None):
    """abub_abf_encode_dev: pixels u8 (any shape; frames of W * H bytes anywhere in it), src: byte offset of each frame
    (any alignment), out u8 (None: nframes * abub_abf_file_bound(W, H), rounded up to 16 per file; out_cap: the kernels may
    write only that many bytes of it, default all) ->
    (files int64 [n, 3] of (off, len, status) on the host, total, out).  File f is out[off:off + len], the bytes
    host.abf_encode gives the frame; status: 0, ABUB_ABF_ENC_E_SRC = 1, ABUB_ABF_ENC_E_CAP = 2 (total stays true)."""
    return _encode("abub_abf_encode_dev", "abub_abf_file_bound", "abub_abf_encode_scratch_bytes", pixels, src, W, H, out, scratch, out_cap)


def png_encode(pixels, src, W, H, out=None, scratch=None, out_cap=None):
    """abub_png_encode_dev: the arguments and results of abf_encode; file f is out[off:off + len], the canonical Huffman-only
    PNG host.png_huff_encode gives the frame (out=None: nframes * abub_png_file_bound(W, H), rounded up to 16 per file)."""
    return _encode("abub_png_encode_dev", "abub_png_file_bound", "abub_png_encode_scratch_bytes", pixels, src, W, H, out, scratch, out_cap)


def frames_compare(a, b, pairs, frame_bytes, a_bytes=None, b_bytes=None, results=None):
    """abub_frames_compare_dev: a, b u8 (any shape, may be the same tensor; frames of frame_bytes bytes anywhere in them),
    pairs: [n, 2] byte offsets of the two frames of each pair (any alignment); a_bytes / b_bytes: the sizes the kernel is
    told (default: the tensors'); results: int32 device tensor of at least 4 * n elements, written in place (None: a new
    one) -> int64 [n, 4] on the host: (status, ndiff, first, max_abs); status 0 or ABUB_CMP_E_RANGE = 1, first
    0xffffffff when ndiff == 0."""
    import numpy as np
    _need_cuda(a, b, results)
    offs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n = len(offs)
    dev = a.device
    d_pairs = torch.from_numpy(np.concatenate([offs, np.zeros((1, 2), np.int64)])).to(dev)
    if results is None:
        results = torch.empty((max(n, 1) * 4,), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().abub_frames_compare_dev(_ptr(a), a.numel() if a_bytes is None else int(a_bytes), _ptr(b),
                                                  b.numel() if b_bytes is None else int(b_bytes), _ptr(d_pairs), n,
                                                  int(frame_bytes), _ptr(results), _stream()), "abub_frames_compare_dev")
    return results.reshape(-1)[:4 * n].cpu().numpy().view(np.uint32).astype(np.int64).reshape(n, 4)


STAT_NONE = 0xFFFFFFFFFFFFFFFF  # abub_stat_job.ref / .model: no reference frame / no model
STAT_COLUMNS = ("status", "min", "max", "n_zero", "n_sat", "n_out", "n_moved", "flags", "sum", "sumsq", "sum_out", "sum_moved")


def frame_stats(frames, jobs, frame_bytes, mu=None, sigma6=None, frames_bytes=None, model_bytes=None, results=None):
    """abub_frame_stats_dev: frames u8 (any shape; frames of frame_bytes bytes anywhere in it), jobs: [n, 3] byte offsets
    (cur, ref, model) of each job's frame and reference frame in `frames` and of its model in mu / sigma6 (u8, the same
    size; any alignment; STAT_NONE or a negative number: no reference frame / no model; mu=None: no job has a model);
    frames_bytes / model_bytes: the sizes the kernel is told (default: the tensors'); results: uint8 device tensor of at
    least 64 * n bytes, 8-byte aligned, written in place (None: a new one) -> uint64 [n, 12] on the host, the columns of
    STAT_COLUMNS; status 0 or ABUB_STAT_E_RANGE = 1, flags bit 0: n_out / sum_out valid, bit 1: n_moved / sum_moved valid."""
    import numpy as np
    _need_cuda(frames, mu, sigma6, results)
    offs = np.array([[STAT_NONE if int(v) < 0 else int(v) for v in row] for row in jobs], dtype=np.uint64).reshape(-1, 3)
    n = len(offs)
    dev = frames.device
    d_jobs = torch.from_numpy(np.concatenate([offs, np.zeros((1, 3), np.uint64)]).view(np.int64)).to(dev)
    if results is None:
        results = torch.empty((max(n, 1) * 64,), dtype=torch.uint8, device=dev)
    if model_bytes is None:
        model_bytes = 0 if mu is None else min(mu.numel(), sigma6.numel())
    _lib.check(_lib.lib().abub_frame_stats_dev(_ptr(frames), frames.numel() if frames_bytes is None else int(frames_bytes),
                                               None if mu is None else _ptr(mu), None if sigma6 is None else _ptr(sigma6),
                                               int(model_bytes), _ptr(d_jobs), n, int(frame_bytes), _ptr(results), _stream()),
               "abub_frame_stats_dev")
    raw = results.reshape(-1)[:64 * n].cpu().numpy()
    return np.concatenate([raw.view(np.uint32).reshape(n, 16)[:, :8].astype(np.uint64), raw.view(np.uint64).reshape(n, 8)[:, 4:]],
                          axis=1)


SHIFT_E_RANGE = 1


def _model_jobs(entry, frames, mu, jobs, args, frames_bytes, model_bytes, status, out, shape, dtype, view, job_words=2):
    """The shared body of frame_shift, frame_shift_cells, frame_light_cells, frame_focus_cells and frame_noise_cells, whose
    entries take (frames, frames_bytes, mu, model_bytes, jobs, n, *args, status, out, stream): the [n, job_words] jobs tensor
    (a negative offset: UINT64_MAX) with a spare row behind it, a new status tensor preset to 0x5A5A5A5A and a new `out` of `dtype` preset to -1 where none is given, the
    call checked -> (status int64 [n] on the host, out as `view` [n, *shape] on the host)."""
    import numpy as np
    _need_cuda(frames, mu, status, out)
    offs = np.array([[int(v) & STAT_NONE for v in row] for row in jobs], dtype=np.uint64).reshape(-1, job_words)
    n = len(offs)
    words = n * int(np.prod([max(s, 0) for s in shape]))
    dev = frames.device
    d_jobs = torch.from_numpy(np.concatenate([offs, np.zeros((1, job_words), np.uint64)]).view(np.int64)).to(dev)
    if status is None:
        status = torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    if out is None:
        out = torch.full((max(words, 1),), -1, dtype=dtype, device=dev)
    _lib.check(getattr(_lib.lib(), entry)(_ptr(frames), frames.numel() if frames_bytes is None else int(frames_bytes), _ptr(mu),
                                          mu.numel() if model_bytes is None else int(model_bytes), _ptr(d_jobs), n, *args, _ptr(status),
                                          _ptr(out), _stream()), entry)
    return (status.reshape(-1)[:n].cpu().numpy().astype(np.int64),
            out.reshape(-1)[:words].cpu().numpy().view(view).reshape(n, *shape))


def frame_shift(frames, mu, jobs, W, H, R, frames_bytes=None, model_bytes=None, status=None, sad=None):
    """abub_frame_shift_dev: frames / mu u8 device tensors (any shape), jobs: [n, 2] byte offsets (cur, model) of each job's
    W x H frame in `frames` and of its model plane in `mu` (any alignment); R: the radius, 1 to 8; frames_bytes /
    model_bytes: the sizes the kernel is told (default: the tensors'); status: int32 device tensor of at least n words, sad:
    int64 device tensor of at least n * (2 R + 1)^2 words, both written in place (None: new ones)
    -> (status int64 [n] on the host: 0 or SHIFT_E_RANGE; the surfaces, uint64 [n, 2 R + 1, 2 R + 1] on the host, entry
    [dy + R, dx + R])."""
    D = 2 * int(R) + 1
    return _model_jobs("abub_frame_shift_dev", frames, mu, jobs, (int(W), int(H), int(R)), frames_bytes, model_bytes, status, sad,
                       (D, D), torch.int64, "uint64")


FIELD_CELL = 128  # ABUB_FIELD_CELL of include/abub_hip.h


def field_grid(W, H, R):
    """abub_frame_cells_grid, the one copy of the grid's rule (no device): -> (ncx, ncy, x0, y0), the whole 128 x 128 cells
    of a W x H frame's interior at radius R and the first cell's first pixel; ncx * ncy == 0: the frame has no field."""
    import ctypes
    out = [ctypes.c_int() for _ in range(4)]
    _lib.check(_lib.lib().abub_frame_cells_grid(int(W), int(H), int(R), *[ctypes.byref(v) for v in out]), "abub_frame_cells_grid")
    return tuple(v.value for v in out)


def frame_shift_cells(frames, mu, jobs, W, H, R, frames_bytes=None, model_bytes=None, status=None, sad=None):
    """abub_frame_shift_cells_dev: the arguments of frame_shift; sad: int32 device tensor of at least
    n * ncy * ncx * (2 R + 1)^2 words, written in place (None: a new one)
    -> (status int64 [n] on the host: 0 or SHIFT_E_RANGE; the surfaces, uint32 [n, ncy, ncx, 2 R + 1, 2 R + 1] on the
    host, entry [dy + R, dx + R] of cell (cx, cy))."""
    D = 2 * int(R) + 1
    ncx, ncy, _, _ = field_grid(W, H, R)
    return _model_jobs("abub_frame_shift_cells_dev", frames, mu, jobs, (int(W), int(H), int(R)), frames_bytes, model_bytes, status, sad,
                       (ncy, ncx, D, D), torch.int32, "uint32")


LIGHT_WORDS = 6  # ABUB_LIGHT_WORDS of include/abub_hip.h


def frame_light_cells(frames, mu, jobs, W, H, x0, y0, ncx, ncy, frames_bytes=None, model_bytes=None, status=None, rec=None):
    """abub_frame_light_cells_dev: frames, mu and jobs as for frame_shift; the grid of ncx x ncy cells of 128 x 128 pixels
    from (x0, y0); rec: int32 device tensor of at least n * ncy * ncx * 6 words, written in place (None: a new one)
    -> (status int64 [n] on the host: 0 or SHIFT_E_RANGE; the records, uint32 [n, ncy, ncx, 6] on the host: the sums of p,
    p^2, p m and |p - m|, the pixels with p == 0 and with p == 255)."""
    return _model_jobs("abub_frame_light_cells_dev", frames, mu, jobs, (int(W), int(H), int(x0), int(y0), int(ncx), int(ncy)),
                       frames_bytes, model_bytes, status, rec, (int(ncy), int(ncx), LIGHT_WORDS), torch.int32, "uint32")


FOCUS_WORDS = 5  # ABUB_FOCUS_WORDS of include/abub_hip.h


def frame_focus_cells(frames, mu, jobs, W, H, x0, y0, ncx, ncy, frames_bytes=None, model_bytes=None, status=None, rec=None):
    """abub_frame_focus_cells_dev: frames, mu and jobs as for frame_shift; the grid of ncx x ncy cells of 128 x 128 pixels
    from (x0, y0), with a ring of one pixel inside the frame; rec: int32 device tensor of at least n * ncy * ncx * 5 words,
    written in place (None: a new one) -> (status int64 [n] on the host: 0 or SHIFT_E_RANGE; the records, int32
    [n, ncy, ncx, 5] on the host: the sums of gx^2, gy^2, gx hx and gy hy, the pixels with p == 0 or p == 255)."""
    return _model_jobs("abub_frame_focus_cells_dev", frames, mu, jobs, (int(W), int(H), int(x0), int(y0), int(ncx), int(ncy)),
                       frames_bytes, model_bytes, status, rec, (int(ncy), int(ncx), FOCUS_WORDS), torch.int32, "int32")


NOISE_WORDS = 6  # ABUB_NOISE_WORDS of include/abub_hip.h


def frame_noise_cells(frames, sigma6, jobs, W, H, x0, y0, ncx, ncy, frames_bytes=None, model_bytes=None, status=None, rec=None):
    """abub_frame_noise_cells_dev: frames and sigma6 u8 device tensors (any shape), jobs: [n, 3] byte offsets (cur, ref,
    model) of each job's W x H frame and reference frame in `frames` and of its plane in `sigma6` (any alignment; STAT_NONE
    or a negative number is out of range like any other offset past the buffer); the grid of ncx x ncy cells of 128 x 128
    pixels from (x0, y0); rec: int32 device tensor of at least n * ncy * ncx * 6 words, written in place (None: a new one)
    -> (status int64 [n] on the host: 0 or SHIFT_E_RANGE; the records, int32 [n, ncy, ncx, 6] on the host: n_over, n_clip,
    s1_in, s2_in, sad, s2_all)."""
    return _model_jobs("abub_frame_noise_cells_dev", frames, sigma6, jobs, (int(W), int(H), int(x0), int(y0), int(ncx), int(ncy)),
                       frames_bytes, model_bytes, status, rec, (int(ncy), int(ncx), NOISE_WORDS), torch.int32, "int32", job_words=3)


LINES_ROW_WORDS = 5  # ABUB_LINES_ROW_WORDS of include/abub_hip.h
LINES_COL_WORDS = 3  # ABUB_LINES_COL_WORDS


def frame_lines(frames, mu, jobs, W, H, frames_bytes=None, model_bytes=None, status=None, rows=None, cols=None):
    """abub_frame_lines_dev: frames and mu u8 device tensors (any shape), jobs: [n, 3] byte offsets (cur, ref, model) of each
    job's W x H frame and reference frame in `frames` and of its plane in `mu` (any alignment; ref STAT_NONE or negative: no
    reference frame); rows / cols: int32 device tensors of at least n * H * 5 and n * W * 3 words, written in place (None:
    new ones) -> (status int64 [n] on the host: 0 or SHIFT_E_RANGE; rows uint32 [n, H, 5] on the host: sum p, sum |p - mu|,
    n_clip, sum |p - r|, n_same; cols uint32 [n, W, 3]: the first three per column)."""
    import numpy as np
    _need_cuda(frames, mu, status, rows, cols)
    offs = np.array([[int(v) & STAT_NONE for v in row] for row in jobs], dtype=np.uint64).reshape(-1, 3)
    n, W, H = len(offs), int(W), int(H)
    dev = frames.device
    d_jobs = torch.from_numpy(np.concatenate([offs, np.zeros((1, 3), np.uint64)]).view(np.int64)).to(dev)
    if status is None:
        status = torch.full((max(n, 1),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    if rows is None:
        rows = torch.full((max(n * H * LINES_ROW_WORDS, 1),), -1, dtype=torch.int32, device=dev)
    if cols is None:
        cols = torch.full((max(n * W * LINES_COL_WORDS, 1),), -1, dtype=torch.int32, device=dev)
    assert rows.numel() >= n * H * LINES_ROW_WORDS and cols.numel() >= n * W * LINES_COL_WORDS and status.numel() >= n
    _lib.check(_lib.lib().abub_frame_lines_dev(_ptr(frames), frames.numel() if frames_bytes is None else int(frames_bytes), _ptr(mu),
                                               mu.numel() if model_bytes is None else int(model_bytes), _ptr(d_jobs), n, W, H,
                                               _ptr(status), _ptr(rows), _ptr(cols), _stream()), "abub_frame_lines_dev")
    return (status.reshape(-1)[:n].cpu().numpy().astype(np.int64),
            rows.reshape(-1)[:n * H * LINES_ROW_WORDS].cpu().numpy().view(np.uint32).reshape(n, H, LINES_ROW_WORDS),
            cols.reshape(-1)[:n * W * LINES_COL_WORDS].cpu().numpy().view(np.uint32).reshape(n, W, LINES_COL_WORDS))


ACT_PLANES = ("n_zero","n_sat", "n_out", "sum_out", "n_moved", "sum_moved")
ACT_E_RANGE = 1
ACT_PIXELS_PER_THREAD = 8  # AC_PX of csrc/abub_stats.hip: the run of pixels a thread owns


def pixel_activity(frames, jobs, frame_bytes, planes, mu=None, sigma6=None, plane_stride=None, frames_bytes=None):
    """abub_pixel_activity_dev, one camera's jobs: frames u8 (any shape; frames of frame_bytes bytes anywhere in it), jobs:
    [n, 2] byte offsets (cur, ref) into `frames` (STAT_NONE or a negative number: no reference frame), mu / sigma6: the
    camera's model (u8 tensors or views, any alignment) or both None; planes: uint32 device tensor, 16-byte aligned, of at
    least 5 * plane_stride + frame_bytes words (plane_stride: default its size / 6), ADDED to in place.
    -> the status word: 0, or ACT_E_RANGE if a job named a stream that runs past frames_bytes (default: the tensor's
    size) and was left out."""
    import numpy as np
    _need_cuda(frames, mu, sigma6, planes)
    offs = np.array([[STAT_NONE if int(v) < 0 else int(v) for v in row] for row in jobs], dtype=np.uint64).reshape(-1, 2)
    n = len(offs)
    dev = frames.device
    d_jobs = torch.from_numpy(np.concatenate([offs, np.zeros((1, 2), np.uint64)]).view(np.int64)).to(dev)
    status = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    if plane_stride is None:
        plane_stride = planes.numel() // 6
    _lib.check(_lib.lib().abub_pixel_activity_dev(_ptr(frames), frames.numel() if frames_bytes is None else int(frames_bytes),
                                                  _ptr(mu), _ptr(sigma6), _ptr(d_jobs), n, int(frame_bytes), _ptr(planes),
                                                  int(plane_stride), _ptr(status), _stream()), "abub_pixel_activity_dev")
    return int(status.item()) if n else 0


def peek_items(rows):
    """rows of (diff, frame, thr_out, pres_out, thr, rect_begin, rect_count) -> the abub_peek_item records as a uint8 host
    array (48 bytes each)."""
    import numpy as np
    dt = np.dtype([("diff", "<u8"), ("frame", "<u8"), ("thr_out", "<u8"), ("pres_out", "<u8"), ("thr", "<i4"),
                   ("rect_begin", "<i4"), ("rect_count", "<i4"), ("reserved", "<i4")])
    rec = np.zeros(len(rows), dtype=dt)
    for k, r in enumerate(rows):
        rec[k] = tuple(int(v) for v in r) + (0,)
    return rec.view(np.uint8).reshape(-1)


def peek_planes(diff, frames, items, rects, W, H, out, diff_bytes=None, frames_bytes=None, out_bytes=None):
    """abub_peek_planes_dev: diff, frames u8 (any shape; D planes and frames of W * H bytes anywhere in them), items: rows of
    (diff, frame, thr_out, pres_out, thr, rect_begin, rect_count) with byte offsets into diff / frames / out (thr_out and
    pres_out multiples of 16), rects: [m, 4] of (x, y, w, h); out u8, written in place: per item the thresholded plane
    (255 where D > thr) at thr_out and the trigger frame with its rectangles drawn at pres_out.  *_bytes: the sizes the
    kernel is told (default: the tensors').  -> int32 [n] on the host: 0, or ABUB_PEEK_E_SRC = 1, _DST = 2, _RECT = 3 (then
    not a byte of the item's planes is written)."""
    import numpy as np
    _need_cuda(diff, frames, out)
    dev = out.device
    rows = list(items)
    n = len(rows)
    rc = np.asarray(rects, dtype=np.int64).reshape(-1, 4).astype(np.int32)
    m = len(rc)
    d_items = torch.from_numpy(np.concatenate([peek_items(rows), np.zeros(48, np.uint8)])).to(dev)
    d_rects = torch.from_numpy(np.concatenate([rc, np.zeros((1, 4), np.int32)])).to(dev)
    status = torch.full((max(n, 1),), 99, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().abub_peek_planes_dev(_ptr(diff), diff.numel() if diff_bytes is None else int(diff_bytes), _ptr(frames),
                                               frames.numel() if frames_bytes is None else int(frames_bytes), _ptr(d_items), n,
                                               _ptr(d_rects), m, W, H, _ptr(out),
                                               out.numel() if out_bytes is None else int(out_bytes), _ptr(status), _stream()),
               "abub_peek_planes_dev")
    return status[:n].cpu().numpy()


def match_terms(frames, frame_idx, tmpl, out=None):
    """Exact CCORR terms (abub_match_ccorr_batch_dev): frames u8 [N,H,W] (any slab of frames), frame_idx int32 [njobs]
    (frame of each job), tmpl u8 [th,tw] -> (num, wsum2), each int64 [njobs, H-th+1, W-tw+1] holding the u64 sums.
    out: (num, wsum2) of that shape and type to write in place (default: fresh tensors)."""
    _need_cuda(frames, frame_idx, tmpl)
    H, W = frames.shape[-2:]
    th, tw = tmpl.shape
    n = frame_idx.numel()
    shape = (n, H - th + 1, W - tw + 1)
    if out is None:
        num = torch.empty(shape, dtype=torch.int64, device=frames.device)
        w2 = torch.empty_like(num)
    else:
        num, w2 = out
        _need_cuda(num, w2)
        assert num.dtype == w2.dtype == torch.int64 and tuple(num.shape) == tuple(w2.shape) == shape
    _lib.check(_lib.lib().abub_match_ccorr_batch_dev(_ptr(frames), W, H, _ptr(frame_idx), n, _ptr(tmpl), tw, th,
                                                     _ptr(num), _ptr(w2), _stream()), "abub_match_ccorr_batch_dev")
    return num, w2


def match_best(frames, frame_idx, tmpl, scratch=None, out=None):
    """Best template position per job, computed on the device (abub_match_best_batch_dev) -> float32 [njobs, 2] (x, y).
    scratch: u8, contiguous, 256-byte aligned, at least abub_match_best_scratch_bytes; out: float32, contiguous, at least
    2 * njobs elements, written in place and returned (both default to fresh tensors)."""
    _need_cuda(frames, frame_idx, tmpl)
    H, W = frames.shape[-2:]
    th, tw = tmpl.shape
    n = frame_idx.numel()
    need = _lib.lib().abub_match_best_scratch_bytes(W, H, tw, th, n)
    if scratch is None:
        scratch = torch.empty(max(need, 1), dtype=torch.uint8, device=frames.device)
    if out is None:
        out = torch.empty((n, 2), dtype=torch.float32, device=frames.device)
    else:
        _need_cuda(out)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= 2 * n
    _lib.check(_lib.lib().abub_match_best_batch_dev(_ptr(frames), W, H, _ptr(frame_idx), n, _ptr(tmpl), tw, th,
                                                    _ptr(out), _ptr(scratch), scratch.numel(), _stream()),
               "abub_match_best_batch_dev")
    return out


# ---- K7: descriptors and the localizer's decisions on K5's polygons (abub_localize.hip) -------------------------
LOC_DONE, LOC_LIMIT, LOC_SLOT, LOC_BAD_FRAME, LOC_BELLOWS, LOC_INCOMPLETE = 0, 1, 2, 3, 4, 5


def localize_limits():
    """(max_contours, max_bubbles) of K7b: a stack with more contours in a slot, or more bubbles, keeps the host route."""
    import ctypes as C
    mc, mb = C.c_int(0), C.c_int(0)
    _lib.check(_lib.lib().abub_localize_limits(C.byref(mc), C.byref(mb)), "abub_localize_limits")
    return mc.value, mb.value


def desc_dtype():
    """numpy dtype of one abub_contour_desc record"""
    import numpy as np
    return np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("area", "<f8"), ("radius", "<f8"), ("m00", "<f8"),
                     ("m10", "<f8"), ("m01", "<f8"), ("cx", "<f4"), ("cy", "<f4"), ("gx", "<f4"), ("gy", "<f4"), ("npts", "<u4"),
                     ("reserved", "<u4")])


def describe_contours(tc, cont_cap=None, pts_cap=None, desc_cap=None):
    """K7a (abub_describe_contours_dev) on the dict trace_contours() returned -> uint8 device tensor [desc_cap, 80], one
    abub_contour_desc per contour of the list (desc_records() reads it on the host).  The capacities default to the sizes
    of the list's tensors."""
    status, cont_off, npts, pt_off, pts = tc["status"], tc["cont_off"], tc["cont_npts"], tc["pt_off"], tc["pts"]
    _need_cuda(status, cont_off, npts, pt_off, pts)
    n = status.numel()
    cont_cap = int(npts.numel()) if cont_cap is None else int(cont_cap)
    pts_cap = int(pts.numel()) if pts_cap is None else int(pts_cap)
    desc_cap = cont_cap if desc_cap is None else int(desc_cap)
    desc = torch.zeros((max(desc_cap, 1), 80), dtype=torch.uint8, device=status.device)
    _lib.check(_lib.lib().abub_describe_contours_dev(_ptr(status), _ptr(cont_off), _ptr(npts), cont_cap, _ptr(pt_off), _ptr(pts),
                                                     pts_cap, n, _ptr(desc), desc_cap, _stream()), "abub_describe_contours_dev")
    return desc


def desc_records(desc, n=None):
    """the records of describe_contours() as a numpy structured array (desc_dtype)"""
    a = desc.cpu().numpy().reshape(-1).view(desc_dtype())
    return a if n is None else a[:n]


def localize_stacks(stacks, masks, slot_status, cont_off, desc, ndesc=None, rect_cap=None, track_cap=None, guard=0):
    """K7b (abub_localize_stacks_dev): the localizer's decisions per stack in one launch.  stacks: a list of dicts with cam,
    genesis (slot) and track (slots in frame order), optionally bad; masks: per camera (fiducial, bellows), each a uint8
    device tensor [h, w] or None; slot_status / cont_off: of trace_contours(); desc: of describe_contours().
    -> (list of dicts with status, nrects, nbubbles, rects (list of (x, y, w, h), None when the list was too small) and
    bubbles (per bubble the record indices of its descriptors, None when the list was too small), totals (rects, track
    dwords) that the launch would have needed, (rects, tracks) as numpy arrays with `guard` more entries than the
    capacities, filled with -1 before the launch)."""
    import ctypes as C
    _need_cuda(slot_status, cont_off, desc)
    n, nc = len(stacks), len(masks)
    st = (_lib.LocStack * max(n, 1))()
    mk = (_lib.LocMask * max(nc, 1))()
    for i, s in enumerate(stacks):
        st[i].cam, st[i].genesis, st[i].ntrack, st[i].bad = s["cam"], s["genesis"], len(s["track"]), int(s.get("bad", 0))
        for k, t in enumerate(s["track"][:_lib.LOC_MAXTRACK]):
            st[i].track[k] = t
    for c, (fid, bel) in enumerate(masks):
        _need_cuda(fid, bel)
        mk[c].fid, mk[c].bel = _ptr(fid), _ptr(bel)
        mk[c].fh, mk[c].fw = (fid.shape if fid is not None else (0, 0))
        mk[c].bh, mk[c].bw = (bel.shape if bel is not None else (0, 0))
    dev = desc.device
    L = _lib.lib()
    ndesc = int(desc.shape[0]) if ndesc is None else int(ndesc)
    mc, mb = localize_limits()
    rect_cap = max(n * mc, 1) if rect_cap is None else int(rect_cap)
    track_cap = max(n * mb * (_lib.LOC_MAXTRACK + 2), 1) if track_cap is None else int(track_cap)
    scratch = torch.empty((max(int(L.abub_localize_scratch_bytes(n, nc)), 1),), dtype=torch.uint8, device=dev)
    out = torch.zeros((max(n, 1), 8), dtype=torch.int32, device=dev)
    rects = torch.full((rect_cap + guard, 4), -1, dtype=torch.int32, device=dev)
    tracks = torch.full((track_cap + guard,), -1, dtype=torch.int32, device=dev)
    totals = torch.zeros((2,), dtype=torch.int32, device=dev)
    _lib.check(L.abub_localize_stacks_dev(C.addressof(st), n, C.addressof(mk), nc, _ptr(slot_status), _ptr(cont_off),
                                          slot_status.numel(), _ptr(desc), ndesc, _ptr(scratch), scratch.numel(), _ptr(out),
                                          _ptr(rects), rect_cap, _ptr(tracks), track_cap, _ptr(totals), _stream()),
               "abub_localize_stacks_dev")
    rows = out.cpu().numpy()  # (synchronises: the host arrays above stay alive until here)
    R, T, tot = rects.cpu().numpy(), tracks.cpu().numpy(), [int(v) for v in totals.cpu().numpy()]
    res = []
    for i in range(n):
        status, nrects, roff, nbub, ntr, toff = (int(v) for v in rows[i, :6])
        r = {"status": status, "nrects": nrects, "nbubbles": nbub, "rects": None, "bubbles": None,
             "rect_off": roff, "track_off": toff, "ntrack": ntr}
        if status == 0:
            if roff + nrects <= rect_cap:
                r["rects"] = [tuple(int(v) for v in R[roff + k]) for k in range(nrects)]
            if toff + ntr <= track_cap:
                o, bub = toff, []
                for _ in range(nbub):
                    m = int(T[o])
                    bub.append([int(v) for v in T[o + 1:o + 1 + m]])
                    o += 1 + m
                r["bubbles"] = bub
        res.append(r)
    return res, tot, (R, T)
