"""abub3hs campaigns (--runs / --run-list, abub::RunCampaign): many runs in one process.  On CPU the argument checks that
come before any HIP call; on the GPU every run's file must equal the oracle's text and the file of a single -r
invocation, with the pipeline reused across runs of one shape."""
import os
import re
import shutil
import zipfile

import numpy as np
import pytest
from PIL import Image

from autobub3hs_amd import host, synth
from test_cli import run_cli


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


# ---- CPU: refused before anything runs ------------------------------------------------------------------------------

def test_duplicate_run_id_is_refused(tmp_path):
    rc, _, err = run_cli(["-d", str(tmp_path), "--runs", "20200101_0,20200101_1,20200101_0", "-o", str(tmp_path)])
    assert rc == 255 and "duplicate run ID '20200101_0'" in err


def test_r_with_runs_is_refused(tmp_path):
    rc, _, err = run_cli(["-d", str(tmp_path), "-r", "20200101_0", "--runs", "20200101_1", "-o", str(tmp_path)])
    assert rc == 255 and "-r cannot be combined with --runs or --run-list" in err


def test_missing_run_list_file(tmp_path):
    rc, _, err = run_cli(["-d", str(tmp_path), "--run-list", str(tmp_path / "nope.txt"), "-o", str(tmp_path)])
    assert rc == 255 and "--run-list: cannot read" in err


def test_event_with_two_runs_is_refused(tmp_path):
    rc, _, err = run_cli(["-d", str(tmp_path), "--runs", "20200101_0,20200101_1", "-e", "1", "-o", str(tmp_path)])
    assert rc == 255 and "-e/--event cannot be used with more than one run" in err


def test_per_event_with_two_runs_is_refused(tmp_path):
    lst = tmp_path / "runs.txt"
    lst.write_text("# a campaign\n20200101_0\n\n20200101_1  # second\n")
    rc, _, err = run_cli(["-d", str(tmp_path), "--run-list", str(lst), "--per-event", "-o", str(tmp_path)])
    assert rc == 255 and "--per-event cannot be used with more than one run" in err


# ---- GPU -------------------------------------------------------------------------------------------------------------

ENV = {"ABUB_THREADS": "4", "ABUB_NUM_CAMS": "2"}


def env_of(env):
    """ENV updated by env; a value of None leaves the variable out"""
    e = dict(ENV)
    e.update(env or {})
    return {k: v for k, v in e.items() if v is not None}


def moving_object(img):
    out = img.copy()
    out[20:60, 40:120] = 255  # between frames 0 and 1: the pair's entropy is far above the training veto's threshold
    return out


def make_seeded_run(root, oracle, run_id, seed, vetoed=(), W=320, H=128, F=41, ncams=2, nev=5):
    """_make_run (tests/test_cli.py) with a seed of its own: the frames of every event differ from run to run, and the
    events in `vetoed` carry a moving object between frames 0 and 1, so the run trains on 2 * (nev - len(vetoed)) frames
    per camera.  Same irregular stacks (event 3 / cam 1: truncated frame 7; event 4 / cam 0: 20 frames).  Returns the
    oracle's text."""
    rd = os.path.join(root, run_id)
    stacks, ok = {}, {}
    for e in range(nev):
        for c in range(ncams):
            s0 = 5000 + 100 * seed + e
            spec = synth.random_spec(W, H, F, s0, c, p_none=0.2, margin=20)
            st = synth.render_event(W, H, spec, s0, c)
            if e in vetoed:
                st[1] = moving_object(st[1])
            if (e, c) == (4, 0):
                st = st[:20]
            stacks[(e, c)] = st
            ok[(e, c)] = np.ones(len(st), np.uint8)
            d = os.path.join(rd, str(e), "Images")
            os.makedirs(d, exist_ok=True)
            for k in range(len(st)):
                path = os.path.join(d, f"cam{c}_image{30 + k}.png")
                Image.fromarray(st[k]).save(path)
                if (e, c, k) == (3, 1, 7):
                    raw = open(path, "rb").read()
                    open(path, "wb").write(raw[: len(raw) // 2])
                    ok[(e, c)][k] = 0
    models = []
    for c in range(ncams):
        for e in range(nev):
            vetoed_here = oracle.pair_entropy16(stacks[(e, c)][1], stacks[(e, c)][0]) > 0.0005
            assert vetoed_here == (e in vetoed), (run_id, e, c)
        tr = np.concatenate([stacks[(e, c)][:2] for e in range(nev) if e not in vetoed])
        mu, sg = oracle.welford(tr)
        models.append((mu, sg, len(tr)))
    blocks = []
    for e in range(nev):
        ans, staged = [], []
        for c in range(ncams):
            a = oracle.Analyzer(stacks[(e, c)], *models[c], frame_ok=ok[(e, c)])
            staged.append(a.any_cam_analysis()[0])
            ans.append(a)
        blocks.append(oracle.format_event(ans, staged, run_id, e, 30))
        for a in ans:
            a.close()
    return oracle.format_header() + "".join(blocks)


def make_runs(tmp_path, oracle, ids, seeds=None, vetoed=None, **kw):
    """runs under tmp_path/data, seed i for ids[i] unless `seeds` says otherwise; {id: expected text}"""
    data = os.path.join(str(tmp_path), "data")
    exp = {}
    for i, rid in enumerate(ids):
        exp[rid] = make_seeded_run(data, oracle, rid, seeds[i] if seeds else i, (vetoed or {}).get(rid, ()), **kw)
    return data, exp


def campaign(tmp_path, tag, data, ids, extra=(), env=None, expect_rc=0):
    out = os.path.join(str(tmp_path), "out_" + tag)
    os.makedirs(out)
    lst = os.path.join(str(tmp_path), tag + ".txt")
    with open(lst, "w") as f:
        f.write("# runs\n" + "\n".join(ids) + "\n")
    e = env_of(env)
    rc, so, se = run_cli(["-d", data, "--run-list", lst, "-o", out, "-D", "40l-19"] + list(extra), env=e)
    assert rc == (expect_rc & 0xFF), (tag, rc, so[-3000:], se[-3000:])
    m = re.search(r"campaign: (\d+) runs, .*pipelines built (\d+); not run: (.*)", so)
    assert m, so[-3000:]
    return out, so, int(m.group(2))


def single(tmp_path, data, rid, extra=(), env=None):
    out = os.path.join(str(tmp_path), "single_" + rid)
    os.makedirs(out, exist_ok=True)
    e = env_of(env)
    rc, so, se = run_cli(["-d", data, "-r", rid, "-o", out, "-D", "40l-19"] + list(extra), env=e)
    return rc, open(os.path.join(out, f"abub3hs_{rid}.txt")).read()


def read(out, rid):
    return open(os.path.join(out, f"abub3hs_{rid}.txt")).read()


@pytest.mark.gpu
def test_campaign_of_four_runs(tmp_path, oracle):
    """Four runs of one shape, each with its own frames and model: 10, 8, 4 and 8 training frames per camera.  Run 1 takes
    the pipeline run 0 built (new TrainingSetSizes installed), run 2 (fewer than 6 training frames: the trigger search's
    frame offset is 1, not 2) needs a pipeline of its own, run 3 goes back to the first one."""
    ids = ["20200925_%d" % i for i in range(4)]
    vetoed = {ids[1]: (1,), ids[2]: (1, 2, 3), ids[3]: (0,)}
    data, exp = make_runs(tmp_path, oracle, ids, vetoed=vetoed)
    assert len(set(exp.values())) == 4
    out, so, built = campaign(tmp_path, "four", data, ids)
    assert built == 2 and so.count("batched detect:") == 4
    for rid in ids:
        assert read(out, rid) == exp[rid], rid
    assert single(tmp_path, data, ids[1])[1] == exp[ids[1]]
    # the host Trainer (A/B switch) gives the same files
    out, so, _ = campaign(tmp_path, "host_train", data, ids, env={"ABUB_TRAIN_ON_GPU": "0"})
    for rid in ids:
        assert read(out, rid) == exp[rid], rid
    # two workers sharing the GPU, small batches: every run is cut into several batches dealt to both workers
    out, so, _ = campaign(tmp_path, "gpus2", data, ids, ["--gpus", "2"], env={"ABUB_BATCH_MB": "4"})
    for rid in ids:
        assert read(out, rid) == exp[rid], rid
    # sharded: each shard a campaign, then --merge 2 of every run
    shard_out = os.path.join(str(tmp_path), "out_sharded")
    os.makedirs(shard_out)
    for r in (1, 0):
        e = dict(ENV)
        rc, so, se = run_cli(["-d", data, "--runs", ",".join(ids), "-o", shard_out, "-D", "40l-19", "--gpu-shard", f"{r}/2"],
                             env=e)
        assert rc == 0, (so[-2000:], se[-2000:])
    rc, so, se = run_cli(["--runs", ",".join(ids), "-o", shard_out, "--merge", "2"])
    assert rc == 0, (so, se)
    for rid in ids:
        assert read(shard_out, rid) == exp[rid], rid
    # zip archives
    for rid in ids:
        zip_dir(data, rid)
        os.rename(os.path.join(data, rid), os.path.join(data, rid + "_moved"))
    out, so, built = campaign(tmp_path, "zip", data, ids, ["-z"])
    assert built == 2
    for rid in ids:
        assert read(out, rid) == exp[rid], rid


@pytest.mark.gpu
def test_campaign_with_another_frame_size_in_the_middle(tmp_path, oracle):
    ids = ["20200925_%d" % i for i in range(3)]
    data, exp = make_runs(tmp_path, oracle, [ids[0], ids[2]], seeds=[0, 2], vetoed={ids[2]: (2,)})
    d2, exp2 = make_runs(tmp_path / "other", oracle, [ids[1]], seeds=[1], W=256, H=96)
    shutil.move(os.path.join(d2, ids[1]), os.path.join(data, ids[1]))
    exp.update(exp2)
    out, so, built = campaign(tmp_path, "sizes", data, ids)
    assert built == 2  # the third run takes the first run's pipeline again
    for rid in ids:
        assert read(out, rid) == exp[rid], rid


def zip_dir(data, rid):
    rd = os.path.join(data, rid)
    with zipfile.ZipFile(rd + ".zip", "w", zipfile.ZIP_DEFLATED) as z:
        for dp, dn, fn in os.walk(rd):
            rel = os.path.relpath(dp, data)
            z.writestr(rel + "/", b"")
            for f in sorted(fn):
                z.write(os.path.join(dp, f), os.path.join(rel, f))


@pytest.mark.gpu
def test_campaign_with_missing_and_empty_runs(tmp_path, oracle):
    """Zip archives: a run whose archive does not exist (-5) and an empty archive (-7) in the middle; the later run is still
    written, the campaign exits with -5 (the first nonzero status), every file equals a single -r invocation's.  The same
    with run directories (where a missing directory lists no events)."""
    ids = ["20200925_%d" % i for i in range(2)]
    data, exp = make_runs(tmp_path, oracle, ids, vetoed={ids[1]: (2,)})
    for rid in ids:
        zip_dir(data, rid)
    zipfile.ZipFile(os.path.join(data, "20200925_8.zip"), "w").close()  # an empty archive
    os.makedirs(os.path.join(data, "20200925_8"))                       # an empty run directory
    order = [ids[0], "20200925_7", "20200925_8", ids[1]]                # 20200925_7 does not exist
    for zipped in (True, False):
        extra = ["-z"] if zipped else []
        singles = {rid: single(tmp_path / ("z" if zipped else "d"), data, rid, extra) for rid in order[1:3]}
        assert singles["20200925_8"][0] == (-7 & 0xFF)
        if zipped:
            assert singles["20200925_7"][0] == (-5 & 0xFF)
        out, so, _ = campaign(tmp_path, "gaps_z" if zipped else "gaps_d", data, order, extra,
                              expect_rc=singles["20200925_7"][0])
        assert "not run: none" in so
        for rid in ids:
            assert read(out, rid) == exp[rid], (zipped, rid)
        for rid in order[1:3]:
            assert read(out, rid) == singles[rid][1], (zipped, rid)
    txt = read(os.path.join(str(tmp_path), "out_gaps_z"), "20200925_7").split("\n")
    assert txt[6].startswith("20200925_7  -1  0  0  0  -5  ") and txt[7].startswith("20200925_7  -1  0  0  1  -5  ")


@pytest.mark.gpu
def test_campaign_40l19_camera_count_and_offset_per_run(tmp_path, oracle):
    """without ABUB_NUM_CAMS: 40l-19 runs before 20200713_7 have 2 cameras, later ones 4; before 20200501_1 the frame
    offset is 20, else 30"""
    ids = ["20200430_1", "20200601_1", "20200801_1"]
    data, _ = make_runs(tmp_path, oracle, ids[:2], vetoed={ids[1]: (1,)})
    d4, _ = make_runs(tmp_path / "four", oracle, ids[2:], seeds=[2], ncams=4)
    shutil.move(os.path.join(d4, ids[2]), os.path.join(data, ids[2]))
    assert os.environ.get("ABUB_NUM_CAMS") is None
    out, so, _ = campaign(tmp_path, "40l19", data, ids, env={"ABUB_NUM_CAMS": None})
    for rid in ids:
        rc, txt = single(tmp_path, data, rid, env={"ABUB_NUM_CAMS": None})
        assert rc == 0 and read(out, rid) == txt, rid
    # every event writes one row per camera at least: the camera column (the fifth) reaches 1 or 3
    for rid, ncams in zip(ids, (2, 2, 4)):
        cams = {int(l.split()[4]) for l in read(out, rid).splitlines()[6:] if l.strip()}
        assert cams == set(range(ncams)), (rid, cams)
