"""abub3hs --peek end to end: for every accepted (event, camera) of a small synthetic run the six files of the batched
post-pass decode pixel for pixel to the six files abub3hs --debug 100 writes into DebugPeek/ in the per-event loop; a stack
that ends in -3 gets none.  The run is built so that the oracle, on the CPU, finds a stack accepted at its first trigger,
one accepted only after a retry, one whose boxes include one outside the fiducial mask and one that ends in -3.  The GPU
route and the host route (ABUB_PEEK_GPU=0) write byte-identical files, from a directory and from a stored archive, with
sub-batches of one stack, and with the localize knob; the recon text does not change."""
import os
import subprocess
import zipfile

import numpy as np
import pytest
from PIL import Image

import peekref
from autobub3hs_amd import host, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "autobub3hs_amd", "abub3hs")
W, H, F, C, RUN_ID = 160, 96, 41, 2, "20200925_3"
OUTSIDE, OUTSIDE2, INSIDE = (10, 8), (150, 88), (90, 50)


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


def two_stage(event, cam, first, second):
    """bubble `first` = (cx, cy, t0) and, later, bubble `second`: two renderings of the same noise added up"""
    base = synth.render_event(W, H, synth.EventSpec(F), event, cam).astype(int)
    a = synth.render_event(W, H, synth.EventSpec(F, t0=first[2], bubbles=[(first[0], first[1], 40)]), event, cam).astype(int)
    b = synth.render_event(W, H, synth.EventSpec(F, t0=second[2], bubbles=[(second[0], second[1], 40)]), event, cam).astype(int)
    return np.clip(a + b - base, 0, 255).astype(np.uint8)


def stacks_of_the_run():
    def one(event, cam, t0, bubbles):
        return synth.render_event(W, H, synth.EventSpec(F, t0=t0, bubbles=[(x, y, 40) for x, y in bubbles]), 800 + event, cam)

    st = {}
    st[(0, 0)] = one(0, 0, 14, [(80, 48)])
    st[(0, 1)] = one(0, 1, 16, [(70, 40)])
    st[(1, 0)] = two_stage(801, 0, OUTSIDE + (10,), INSIDE + (24,))  # outside the fiducial ellipse first: a retry
    st[(1, 1)] = synth.render_event(W, H, synth.EventSpec(F), 801, 1)  # nothing happens: -3
    st[(2, 0)] = one(2, 0, 18, [(80, 48), OUTSIDE2])  # one bubble inside the fiducial ellipse and one outside, together
    st[(2, 1)] = one(2, 1, 12, [(60, 44)])
    st[(3, 0)] = synth.render_event(W, H, synth.EventSpec(F), 803, 0)
    st[(3, 1)] = one(3, 1, 20, [(100, 40)])
    return st


class World:
    def __init__(self, tmp, oracle):
        self.tmp = str(tmp)
        self.data = os.path.join(self.tmp, "data")
        self.rd = os.path.join(self.data, RUN_ID)
        self.masks = os.path.join(self.tmp, "masks") + os.sep
        synth.write_masks(self.masks, W, H, C)
        self.stacks = stacks_of_the_run()
        self.nev = 1 + max(e for e, _ in self.stacks)
        for (e, c), st in self.stacks.items():
            d = os.path.join(self.rd, str(e), "Images")
            os.makedirs(d, exist_ok=True)
            for k in range(F):
                Image.fromarray(st[k]).save(os.path.join(d, f"cam{c}_image{30 + k}.png"))
        # what the oracle says about every stack, on the CPU
        self.kinds, self.accepted = {}, []
        for c in range(C):
            tr = np.concatenate([self.stacks[(e, c)][:2] for e in range(self.nev)])
            mu, sg = oracle.welford(tr)
            fid, bel = synth.camera_masks(W, H, c)
            for e in range(self.nev):
                st = self.stacks[(e, c)]
                a = oracle.Analyzer(st, mu, sg, len(tr), fid_mask=fid, bel_mask=bel)
                first = a.find_trigger()["trig"]
                a.close()
                a = oracle.Analyzer(st, mu, sg, len(tr), fid_mask=fid, bel_mask=bel)
                staged, state, bubbles = a.any_cam_analysis()
                a.close()
                kind = set()
                if staged == 0:
                    self.accepted.append((e, c))
                    kind.add("first" if state["trig"] == first else "retry")
                    t = state["trig"]
                    D = oracle.process_frame(st[t], st[max(t - 2, 0)], sg)
                    thr = max(state["loc_thres"], oracle.otsu(oracle.hist256(np.where(D > state["loc_thres"], D, 0))))
                    for xy, _ in oracle.find_contours(np.where(D > thr, 255, 0).astype(np.uint8)):
                        w, h = np.ptp(xy[:, 0]) + 1, np.ptp(xy[:, 1]) + 1
                        if w * h > 10 and not fid[xy[:, 1], xy[:, 0]].any():
                            kind.add("box_outside_fiducial")
                elif staged == -3:
                    kind.add("minus3")
                self.kinds[(e, c)] = kind
        self.zip = None

    def archive(self):
        if self.zip is None:
            self.zip = os.path.join(self.tmp, "zdata")
            os.makedirs(self.zip)
            with zipfile.ZipFile(os.path.join(self.zip, RUN_ID + ".zip"), "w", zipfile.ZIP_STORED) as z:
                for dp, dn, fn in os.walk(self.rd):
                    rel = os.path.relpath(dp, self.data)
                    z.writestr(rel + "/", b"")
                    for f in sorted(fn):
                        z.write(os.path.join(dp, f), os.path.join(rel, f))
        return self.zip

    def cli(self, tag, args=(), env=None, zipped=False, cwd=None):
        out = os.path.join(self.tmp, "out_" + tag)
        os.makedirs(out)
        e = dict(os.environ, ABUB_THREADS="4", ABUB_NUM_CAMS=str(C))
        e.update(env or {})
        p = subprocess.run([EXE] + (["-z"] if zipped else []) + ["-d", self.archive() if zipped else self.data, "-r", RUN_ID, "-o", out,
                                                                  "-D", "40l-19", "-c", self.masks] + list(args),
                           capture_output=True, text=True, env=e, timeout=300, cwd=cwd or self.tmp)
        assert p.returncode == 0, (tag, p.stdout[-3000:], p.stderr[-3000:])
        return open(os.path.join(out, f"abub3hs_{RUN_ID}.txt")).read(), p.stdout

    def peek(self, tag, env=None, zipped=False, args=()):
        d = os.path.join(self.tmp, "peek_" + tag)
        txt, so = self.cli(tag, ["--peek", d] + list(args), env=env, zipped=zipped)
        files = {}
        rd = os.path.join(d, RUN_ID)
        for name in sorted(os.listdir(rd)):
            files[name] = open(os.path.join(rd, name), "rb").read()
        return txt, so, files


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    w = World(tmp_path_factory.mktemp("peek"), oracle)
    os.makedirs(os.path.join(w.tmp, "DebugPeek"))
    w.debug_txt, w.debug_out = w.cli("debug", ["--debug", "100"])  # the per-event loop, images into ./DebugPeek/
    w.gpu_txt, w.gpu_out, w.gpu_files = w.peek("gpu")
    return w


def pixels(data_or_path):
    import io
    return np.asarray(Image.open(io.BytesIO(data_or_path) if isinstance(data_or_path, bytes) else data_or_path).convert("L"))


def test_the_run_holds_the_four_kinds(world):
    kinds = world.kinds
    assert any("first" in k for k in kinds.values()), kinds
    assert any("retry" in k for k in kinds.values()), kinds
    assert any("box_outside_fiducial" in k for k in kinds.values()), kinds
    assert any("minus3" in k for k in kinds.values()), kinds


def test_peek_files_are_the_debug_files_pixel_for_pixel(world):
    test_the_run_holds_the_four_kinds(world)
    want = sorted(n for e, c in world.accepted for n in peekref.file_names(e, c))
    assert sorted(world.gpu_files) == want  # six per accepted stack, none for a stack that ends in -3
    for name in want:
        ref = pixels(os.path.join(world.tmp, "DebugPeek", name))
        assert ref.shape == (H, W)
        got = pixels(world.gpu_files[name])
        assert np.array_equal(got, ref), name
    n = len(world.accepted)
    total = sum(len(v) for v in world.gpu_files.values())
    assert f"peek: {n} stacks, {6 * n} files, {total} bytes, gpu" in world.gpu_out
    assert world.gpu_txt == world.debug_txt
    # the stack with a box outside the fiducial mask: that box is drawn, although its bubble is not in the text
    e, c = [k for k, v in sorted(world.kinds.items()) if "box_outside_fiducial" in v][0]
    fid, _ = synth.camera_masks(W, H, c)
    drawn = pixels(world.gpu_files[f"ev{e}_cam{c}_4_BubbleDetected.png"]) != pixels(world.gpu_files[f"ev{e}_cam{c}_0_TrigFrame.png"])
    assert (drawn & (fid == 0)).any() and (drawn & (fid != 0)).any()


def test_recon_text_is_the_text_without_peek(world):
    txt, so = world.cli("plain")
    assert txt == world.gpu_txt and "peek:" not in so


VARIANTS = {
    "host_route": dict(env={"ABUB_PEEK_GPU": "0"}, says="host"),
    "archive": dict(zipped=True, says="gpu"),
    "archive_host_route": dict(zipped=True, env={"ABUB_PEEK_GPU": "0"}, says="host"),
    "sub_batches_of_one": dict(env={"ABUB_PEEK_BATCH": "1"}, says="gpu"),
    "sub_batches_of_two_host": dict(env={"ABUB_PEEK_BATCH": "2", "ABUB_PEEK_GPU": "0"}, says="host"),
    "small_batches_two_workers": dict(env={"ABUB_BATCH_MB": "2"}, args=["--gpus", "2"], says="gpu"),
    "localize_knob": dict(env={"ABUB_PIPE_LOCALIZE": "1"}, says="gpu"),
    "host_decode": dict(env={"ABUB_GPU_DECODE": "0"}, says="gpu"),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_route_writes_the_same_bytes(world, variant):
    v = VARIANTS[variant]
    txt, so, files = world.peek(variant, env=v.get("env"), zipped=v.get("zipped", False), args=v.get("args", ()))
    assert txt == world.gpu_txt
    assert sorted(files) == sorted(world.gpu_files)
    for name, data in files.items():
        assert data == world.gpu_files[name], name
    assert f"bytes, {v['says']}" in so


def test_python_surface_writes_the_same_files(world, tmp_path):
    run = host.Run(kind="raw", run_folder=world.rd + "/")
    for c in range(C):
        st, tss, mu, sg = run.train(c, shape=(H, W))
        assert st == 0
    out = str(tmp_path) + "/"
    stats = run.run_batched(C, out, RUN_ID, 30, maskdir=world.masks, nthreads=4, decode_threads=4, peek_dir=str(tmp_path / "peek"))
    run.close()
    n = len(world.accepted)
    assert (stats["peek_stacks"], stats["peek_files"], stats["peek_gpu"]) == (n, 6 * n, 1)
    rd = tmp_path / "peek" / RUN_ID
    assert sorted(os.listdir(rd)) == sorted(world.gpu_files)
    for name, data in world.gpu_files.items():
        assert (rd / name).read_bytes() == data, name
    assert stats["peek_bytes"] == sum(len(v) for v in world.gpu_files.values())


def test_vetoed_stack_gets_the_rectangles_after_the_veto(tmp_path, oracle):
    """The small bellows geometry of tests/test_bellows_batched.py as a run on disk: a textured block inside the bellows
    mask creeps from frame 12 on in event 0 and stands still in the others, so every genesis contour of event 0 lies in the
    bellows mask, the veto subtracts the block's motion and the boxes come from what is left.  --peek draws those boxes
    on a D and a cut taken before the veto, exactly as the per-event loop's write-out does."""
    from test_bellows_batched import bellows_event, write_bmp8

    Wb, Hb, Fb, t0, run_id = 200, 120, 24, 12, "20200925_4"
    fr, tex, (bx0, by0) = bellows_event(Wb, Hb, Fb, t0, shift=2)
    stacks = [fr]
    for e in range(1, 4):
        st = synth.render_event(Wb, Hb, synth.EventSpec(Fb, t0=9 + e, bubbles=[(40 + 20 * e, 60, 40)]), 900 + e, 0)
        st[:, by0:by0 + 50, bx0:bx0 + 30] = tex
        stacks.append(st)
    masks = os.path.join(tmp_path, "masks") + os.sep
    os.makedirs(masks)
    bel = np.zeros((Hb, Wb), np.uint8)
    bel[by0 - 10:by0 + 60, bx0 - 10:bx0 + 45] = 255
    write_bmp8(os.path.join(masks, "cam0_bellows_mask.bmp"), bel)
    Image.fromarray(tex).save(os.path.join(masks, "cam0_bellows_template.png"))
    data = os.path.join(tmp_path, "data")
    for e, st in enumerate(stacks):
        d = os.path.join(data, run_id, str(e), "Images")
        os.makedirs(d)
        for k in range(Fb):
            Image.fromarray(st[k]).save(os.path.join(d, f"cam0_image{30 + k}.png"))
    # the oracle: event 0 is accepted at the frame the block starts to move, with the boxes the veto leaves
    tr = np.concatenate([st[:2] for st in stacks])
    mu, sg = oracle.welford(tr)
    a = oracle.Analyzer(fr, mu, sg, len(tr), bel_mask=bel, bel_template=tex)
    staged, state, bubbles = a.any_cam_analysis()
    a.close()
    assert staged == 0 and state["trig"] == t0 and bubbles
    boxes = [tuple(b["desc"][0][k] for k in "xywh") for b in bubbles]
    assert all(bel[y, x] for x, y, w, h in boxes)  # every box of the final round lies in the bellows mask

    def cli(tag, args):
        out = os.path.join(tmp_path, "out_" + tag)
        os.makedirs(out)
        p = subprocess.run([EXE, "-d", data, "-r", run_id, "-o", out, "-D", "40l-19", "-c", masks] + args, capture_output=True, text=True,
                           env=dict(os.environ, ABUB_THREADS="4", ABUB_NUM_CAMS="1"), timeout=300, cwd=tmp_path)
        assert p.returncode == 0, (tag, p.stdout[-3000:], p.stderr[-3000:])
        return open(os.path.join(out, f"abub3hs_{run_id}.txt")).read(), p.stdout

    os.makedirs(os.path.join(tmp_path, "DebugPeek"))
    dbg_txt, dbg_out = cli("debug", ["--debug", "100"])
    assert "Found bubble in bellows mask." in dbg_out
    files = {}
    for tag, env in (("gpu", "1"), ("host", "0")):
        os.environ["ABUB_PEEK_GPU"] = env
        try:
            txt, so = cli(tag, ["--peek", os.path.join(tmp_path, "peek_" + tag)])
        finally:
            os.environ.pop("ABUB_PEEK_GPU", None)
        assert txt == dbg_txt and f"bytes, {tag}" in so
        rd = os.path.join(tmp_path, "peek_" + tag, run_id)
        files[tag] = {n: open(os.path.join(rd, n), "rb").read() for n in sorted(os.listdir(rd))}
    assert files["gpu"] == files["host"]
    for name in peekref.file_names(0, 0):
        assert np.array_equal(pixels(files["gpu"][name]), pixels(os.path.join(tmp_path, "DebugPeek", name))), name
    # the boxes drawn are the veto's: D itself, before the veto, still shows the whole moving block
    trig = pixels(files["gpu"]["ev0_cam0_0_TrigFrame.png"])
    marked = pixels(files["gpu"]["ev0_cam0_4_BubbleDetected.png"])
    assert (marked != trig).any()
    for x, y, w, h in boxes:  # (the oracle's bubbles after the veto: their boxes are among the drawn ones)
        assert marked[y, x] == 255 and marked[y + h - 1, x + w - 1] == 255 and marked[y, x + w - 1] == 255
    D = oracle.process_frame(fr[t0], fr[t0 - 2], sg)
    assert np.array_equal(pixels(files["gpu"]["ev0_cam0_02_OvrThe6Sigma.png"]), D)
