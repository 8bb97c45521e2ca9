"""The numpy restatement of a survey's per-pixel view ("Surveying a run per pixel"): the six activity
planes of abub_pixel_activity_dev / activityAddHost, the three denominators, activity.txt, the .npy file and the quick-look
image.  It builds on tests/surveyref.py for the states and the pairing.  Nothing here calls the code under test."""
import numpy as np

PLANES = ("n_zero", "n_sat", "n_out", "sum_out", "n_moved", "sum_moved")
E_RANGE = 1


def terms(cur, ref=None, mu=None, sigma6=None):
    """what one frame adds to the six planes: int64 [6, n]; without a model planes 2 to 5 get nothing, without a reference
    frame planes 4 and 5"""
    p = np.asarray(cur, np.uint8).reshape(-1).astype(np.int64)
    t = np.zeros((6, p.size), np.int64)
    t[0] = p == 0
    t[1] = p == 255
    if mu is None:
        return t
    s = np.asarray(sigma6, np.uint8).reshape(-1).astype(np.int64)
    out = np.maximum(np.abs(p - np.asarray(mu, np.uint8).reshape(-1).astype(np.int64)) - s, 0)
    t[2], t[3] = out > 0, out
    if ref is not None:
        moved = np.maximum(np.abs(p - np.asarray(ref, np.uint8).reshape(-1).astype(np.int64)) - s, 0)
        t[4], t[5] = moved > 0, moved
    return t


def sigma6_of(sigma):
    return np.minimum(np.asarray(sigma).astype(np.int64) * 6, 255).astype(np.uint8)


def cameras_of(stacks, W, H, models):
    """stacks and models as surveyref.rows_of takes them -> {cam: dict(planes=int64 [6, H * W], frames, frames_model,
    frames_moved)} for every camera with a listed row (a frame that is not the string "missing")"""
    cams = {}
    for _, cam, frames in stacks:
        model = models[cam]
        for i, (_, img) in enumerate(frames):
            if isinstance(img, str):
                continue
            c = cams.setdefault(cam, dict(planes=np.zeros((6, H * W), np.int64), frames=0, frames_model=0, frames_moved=0))
            if img is None or img.shape != (H, W):
                continue
            ref = frames[max(i - 2, 0)][1]
            ref = ref if isinstance(ref, np.ndarray) and ref.shape == (H, W) else None
            c["frames"] += 1
            if model is None:
                c["planes"] += terms(img)
                continue
            c["frames_model"] += 1
            c["frames_moved"] += ref is not None
            c["planes"] += terms(img, ref, model["mu"], sigma6_of(model["sigma"]))
    return cams


def npy_bytes(planes, W, H):
    """NumPy format 1.0 by rule: the header dict padded with spaces and a final newline so that the data starts at a
    multiple of 64, then the six planes as little-endian u32, row-major"""
    head = "{'descr': '<u4', 'fortran_order': False, 'shape': (6, %d, %d), }" % (H, W)
    total = (10 + len(head) + 1 + 63) // 64 * 64
    head += " " * (total - 10 - len(head) - 1) + "\n"
    return b"\x93NUMPY\x01\x00" + len(head).to_bytes(2, "little") + head.encode() + np.asarray(planes).astype("<u4").tobytes()


def moved_image(cam, W, H):
    n, r = cam["planes"][4], cam["frames_moved"]
    return ((255 * n + r - 1) // r if r else 0 * n).astype(np.uint8).reshape(H, W)


def activity_text(cams, W, H, models):
    text = "# abub3hs activity 1\n"
    for c in sorted(cams):
        cam = cams[c]
        z, s, no, so, nm, sm = cam["planes"]
        N, M, R = cam["frames"], cam["frames_model"], cam["frames_moved"]
        text += f"cam {c} w {W} h {H} frames {N} frames_model {M} frames_moved {R}\n"
        dead = int((z == N).sum()) if N else 0
        stuck = int((s == N).sum()) if N else 0
        m10 = int((10 * nm >= R).sum()) if R else 0
        m50 = int((2 * nm >= R).sum()) if R else 0
        text += (f"cam {c} dead {dead} stuck_sat {stuck} ever_out {int((no > 0).sum())} ever_moved {int((nm > 0).sum())} "
                 f"moved_10pct {m10} moved_50pct {m50}\n")
        hot = sorted(np.flatnonzero(nm > 0).tolist(), key=lambda i: (-nm[i], -sm[i], i))[:16]
        for rank, i in enumerate(hot, 1):
            mu = np.asarray(models[c]["mu"]).reshape(-1)
            s6 = sigma6_of(models[c]["sigma"]).reshape(-1)
            text += f"hot {c} {rank} {i % W} {i // W} {nm[i]} {sm[i]} {no[i]} {so[i]} {mu[i]} {s6[i]}\n"
    return text


def files_of(stacks, W, H, models):
    """-> {file name: bytes, or for cam<c>_moved.png the decoded image}: what a planes directory must hold, and nothing else"""
    cams = cameras_of(stacks, W, H, models)
    files = {"activity.txt": activity_text(cams, W, H, models).encode()}
    for c, cam in cams.items():
        files[f"cam{c}_activity.npy"] = npy_bytes(cam["planes"], W, H)
        if models[c] is not None:
            files[f"cam{c}_moved.png"] = moved_image(cam, W, H)
    return files
