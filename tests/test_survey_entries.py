"""The twelve abh_run_survey* entries, called directly.  Run.survey goes through the widest pair alone
(abh_run_survey_focus[_dev]); the ten narrower ones are kept for callers of the C interface, and this is what calls them: each
with every product it can name, on the small run of tests/test_focus_abi.py (300 x 170: a grid of 2 x 1 cells at radius 4),
against Run.survey with the same products: the status, the report, every file byte for byte and the integer counters of
every stats array.  A product an entry cannot name is not written.  On a GPU: the _dev entries against the host entries'
files."""
import ctypes as C
import os

import pytest

from autobub3hs_amd import host
from test_focus_abi import make_focus_run
from test_survey_abi import NCAMS

PRODUCTS = ("planes", "shift", "field", "light", "focus")  # entry number k names the first k of them
ENTRIES = ("abh_run_survey", "abh_run_survey_planes", "abh_run_survey_shift", "abh_run_survey_field", "abh_run_survey_light",
           "abh_run_survey_focus")
CAP = 1 << 16


@pytest.fixture(scope="module", autouse=True)
def _built():
    host.build()


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    return make_focus_run(str(tmp_path_factory.mktemp("entries") / "data"))[0]


def named(out, level):
    """the places of the first `level` products under `out`"""
    return {k: os.path.join(out, k + (".txt" if k == "shift" else "")) for k in PRODUCTS[:level]}


def tree(out):
    return {os.path.relpath(os.path.join(dp, f), out): open(os.path.join(dp, f), "rb").read() for dp, _, fn in os.walk(out) for f in fn}


def call_entry(rd, level, out, device=None):
    """entry number `level` (its _dev twin with a device) -> (rc, the report's text, the integer counters, the files under out)"""
    os.makedirs(out)
    args = [os.path.join(out, "report.txt").encode()]
    for k, path in named(out, level).items():
        args += [path.encode()] + [4] * (k in ("shift", "field"))  # (their radius)
    args += [NCAMS, 4] + [device] * (device is not None)
    st, arrays = (C.c_double * 24)(), [(C.c_double * 5)() for _ in range(level)]
    buf = C.create_string_buffer(CAP)
    run = host.Run("raw", rd + "/", "Images")
    try:
        rc = getattr(host.lib(), ENTRIES[level] + ("_dev" if device is not None else ""))(run._h, *args, st, *arrays, buf, CAP)
    finally:
        run.close()
    counters = [int(v) for v in st[:19]] + [int(st[23])] + [int(v) for a in arrays[:1] for v in a[:2]] + \
               [int(v) for a in arrays[1:] for v in a[:3]]
    return rc, buf.value.decode(), counters, tree(out)


def call_run_survey(rd, level, out):
    """Run.survey with the same products -> the same four"""
    os.makedirs(out)
    run = host.Run("raw", rd + "/", "Images")
    try:
        res, text = run.survey(os.path.join(out, "report.txt"), nthreads=4, ncams=NCAMS, **named(out, level))
    finally:
        run.close()
    counters = [res[k] for k in host.Run._SURVEY_KEYS] + [len(text.encode())] + \
               [res[k] for k in ("plane_rows_kernel", "plane_rows_host")[:2 * (level >= 1)]] + \
               [res[f"{p}_{k}"] for p in PRODUCTS[1:level] for k in ("frames_kernel", "frames_host", "launches")]
    return res["rc"], text, counters, tree(out)


@pytest.fixture(scope="module")
def host_entries(run_dir, tmp_path_factory):
    out = tmp_path_factory.mktemp("host_entries")
    return [call_entry(run_dir, level, str(out / str(level))) for level in range(len(ENTRIES))]


def test_each_host_entry_agrees_with_run_survey(run_dir, host_entries, tmp_path):
    for level, got in enumerate(host_entries):
        want = call_run_survey(run_dir, level, str(tmp_path / str(level)))
        assert got[0] == want[0] == 1, level  # (the truncated file: the survey's status)
        assert got[1] == want[1] and got[1].startswith("# abub3hs survey 1\n") and got[3]["report.txt"].decode() == got[1], level
        assert got[2] == want[2], level
        assert sorted(got[3]) == sorted(want[3]) and all(got[3][f] == want[3][f] for f in got[3]), level
        # nothing of a product the entry cannot name, something of every one it can
        assert {f.split(os.sep)[0] for f in got[3]} == {"report.txt"} | {os.path.basename(p) for p in named("", level).values()}, level
    text = lambda level, f: host_entries[level][3][f].decode()  # noqa: E731
    assert text(1, "planes/activity.txt").startswith("# abub3hs activity 1\n") and text(2, "shift.txt").startswith("# abub3hs shift 1\n")
    for level, k in ((3, "field"), (4, "light"), (5, "focus")):
        assert text(level, f"{k}/{k}.txt").startswith(f"# abub3hs {k} 1\nradius 4 cell 128 grid 2 1 origin 22 21\n"), k
    # a wider entry changes nothing in what a narrower one writes
    for level in range(1, len(ENTRIES)):
        assert all(host_entries[level][3][f] == b for f, b in host_entries[level - 1][3].items()), level


@pytest.mark.gpu
def test_each_dev_entry_writes_the_host_entrys_bytes(run_dir, host_entries, tmp_path):
    for level, want in enumerate(host_entries):
        got = call_entry(run_dir, level, str(tmp_path / str(level)), device=0)
        assert got[0] == want[0] == 1 and got[1] == want[1], level
        assert sorted(got[3]) == sorted(want[3]) and all(got[3][f] == want[3][f] for f in got[3]), level
        assert got[2][14] == 0 and got[2][6] > 0, level  # the device route was taken, and the kernel measured frames
