"""bench.py --gpus N must start its own ranks (the driver may call it without a launcher) and print ONE JSON line.
Rehearsed on CPU: --dry skips every kernel, ABUB_BENCH_BACKEND=gloo replaces RCCL; what runs is the real launch /
barrier / max-over-ranks / gather / report protocol of the multi-GPU path."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=300):
    env = dict(os.environ, ABUB_BENCH_BACKEND="gloo")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_bench_gpus2_launches_itself_and_prints_one_line():
    p = _run(["--gpus", "2", "--dry", "--steps", "3", "--warmup", "1", "--min-seconds", "0.05"])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["scaling"] == "weak"
    t = out["config"]["timing"]
    assert t["blocks"] >= 1 and t["steps_per_block"] == 3
    per_rank = t["ms_per_step_by_rank"]
    assert len(per_rank) == 2 and per_rank[1] > per_rank[0] * 1.5  # the dry straggler (rank 1 sleeps twice as long) shows
    assert out["ms_per_step"] >= per_rank[1] * 0.9                  # a block is as slow as its slowest rank
    assert t["ms_per_step_min"] <= out["ms_per_step"] <= t["ms_per_step_max"]


def test_bench_rejects_a_launcher_with_the_wrong_world_size():
    p = _run(["--gpus", "4", "--dry"], env_extra={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert p.returncode == 2 and "WORLD_SIZE=2" in p.stderr


def test_bench_single_rank_dry():
    p = _run(["--dry", "--steps", "2", "--warmup", "0", "--min-seconds", "0"])
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["n_gpus"] == 1 and out["config"]["timing"]["blocks"] == 1


def test_stdout_is_exactly_one_json_line():
    """The driver reads ONE JSON line from stdout: bench.py moves everything else that lands on fd 1 (the host library's
    printf progress lines) to stderr."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--dry", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1 and json.loads(lines[0])["metric"]


def test_steps_is_the_number_of_timed_steps():
    """Without --min-seconds the timed region is one block of exactly --steps steps."""
    p = _run(["--dry", "--steps", "5", "--warmup", "1"])
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    t = out["config"]["timing"]
    assert out["steps"] == 5 and t["blocks"] == 1 and t["steps_per_block"] == 5
    assert abs(out["ms_per_step"] - t["timed_seconds"] / 5 * 1e3) < 1e-9


def test_dump_outputs_refuses_dry_and_zero_steps():
    assert _run(["--dry", "--dump-outputs", "x"]).returncode == 2
    assert _run(["--dry", "--steps", "0"]).returncode == 2


def test_full_legs_run_only_with_full():
    """A plain run has none of the report's other legs; --full gives each its default size, and an option that sizes one
    of them is refused without --full rather than dropped."""
    import bench

    plain = bench.parse([])
    assert not plain.full and all(getattr(plain, k) == 0 for k in bench.FULL_LEG_SIZES)
    full = bench.parse(["--full"])
    assert all(getattr(full, k) == n and n > 0 for k, n in bench.FULL_LEG_SIZES.items())
    assert bench.parse(["--full", "--latency-steps", "3", "--micro-frames", "0"]).latency_steps == 3
    assert bench.parse(["--micro-frames", "0", "--regime-steps", "0"]).regime_steps == 0
    p = _run(["--dry", "--latency-steps", "3"])
    assert p.returncode == 2 and "--latency-steps" in p.stderr and "--full" in p.stderr


def test_dump_outputs_layout(tmp_path):
    """bench.dump_outputs writes every stack's result (host.Pipeline.result) as float64 arrays."""
    import numpy as np

    import bench
    from autobub3hs_amd import host

    class FakePipe:
        S = 4

        def result(self, s):
            desc = dict(zip(host.DESC_KEYS, [10.0 * s + k for k in range(len(host.DESC_KEYS))]))
            bubbles = [{"desc": [desc, desc], "dzdt": 0.5 * s, "drdt": -0.25}] * (s % 2)
            return s % 3, {"trig": 20 + s, "status": 0, "ok": True, "loc_thres": 7}, bubbles, "" if s else "err"

    bench.dump_outputs(str(tmp_path / "out"), FakePipe(), [5, 9], 2)
    st = np.load(tmp_path / "out" / "stacks.npy")
    de = np.load(tmp_path / "out" / "bubble_desc.npy")
    ra = np.load(tmp_path / "out" / "bubble_rates.npy")
    assert st.dtype == de.dtype == ra.dtype == np.float64
    assert st.tolist() == [[5, 0, 0, 20, 0, 7, 1, 0, 1], [5, 1, 1, 21, 0, 7, 1, 1, 0],
                           [9, 0, 2, 22, 0, 7, 1, 0, 0], [9, 1, 0, 23, 0, 7, 1, 1, 0]]
    assert de.shape == (4, 3 + len(host.DESC_KEYS)) and de[:, :3].tolist() == [[1, 0, 0], [1, 0, 1], [3, 0, 0], [3, 0, 1]]
    assert de[2, 3:].tolist() == [30.0 + k for k in range(len(host.DESC_KEYS))]
    assert ra.tolist() == [[1, 0, 0.5, -0.25], [3, 0, 1.5, -0.25]]
