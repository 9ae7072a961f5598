"""bench.py's rank handling on CPU (no GPU call is made before these checks)."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_must_match_world_size():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "4"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr


def test_launcher_command():
    sys.path.insert(0, REPO)
    import bench
    p = bench.free_port()
    assert 0 < p < 65536


def test_plain_run_defaults(monkeypatch):
    """`--gpus 1 --steps N --warmup W` is the lean run: --full and --dump-outputs are off."""
    sys.path.insert(0, REPO)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_sample_is_fixed_and_within_budget():
    sys.path.insert(0, REPO)
    import bench
    import numpy as np
    rows, envs = bench.dump_sample(256, 4096, 420)
    assert len(envs) == 4096 and rows[-1] == 255 and len(set(rows.tolist())) == len(rows)
    assert len(rows) * len(envs) * 420 <= bench.DUMP_BUDGET_BYTES < 64 * 10**6
    again = bench.dump_sample(256, 4096, 420)
    assert np.array_equal(rows, again[0]) and np.array_equal(envs, again[1])
    rows, envs = bench.dump_sample(256, 65536, 420)
    assert len(envs) == bench.DUMP_MAX_ENVS and np.all(np.diff(envs) > 0) and envs[-1] < 65536
    rows, envs = bench.dump_sample(8, 64, 420)          # a small slab is written whole
    assert rows.tolist() == list(range(8)) and envs.tolist() == list(range(64))
