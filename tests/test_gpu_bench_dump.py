"""`bench.py --dump-outputs DIR` on one GPU: a plain run times exactly --steps steps, runs none of
the --full legs, and writes the last timed step's outputs; two runs with the same arguments write
the same arrays, and the arrays are the oracle's trajectory of the same seeds and action draws."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS, B, STEPS, WARMUP = 256, 64, 4, 1
NAMES = {"obs_i32": np.float64, "obs_i8": np.float32, "obs_f32": np.float32, "masks": np.float32,
         "rewards": np.float64, "term": np.float32, "trunc": np.float32}


def _bench(out_dir, *args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    args = args or ("--steps", str(STEPS), "--warmup", str(WARMUP), "--batch-steps", str(B), "--chunk", "128")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--envs", str(ENVS), *args,
                        "--dump-outputs", str(out_dir)], cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    dirs = [tmp_path_factory.mktemp("dump_a"), tmp_path_factory.mktemp("dump_b")]
    return [(_bench(d), {k: np.load(os.path.join(d, k + ".npy")) for k in NAMES}, d) for d in dirs]


def test_plain_run_is_lean_and_reports_its_steps(runs):
    d, arrays, out_dir = runs[0]
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["full"] is False
    assert d["config"]["env_steps_per_bench_step"] == B * ENVS
    assert d["ms_per_step"] > 0 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    # value and ms_per_step describe the same STEPS timed steps
    assert d["value"] == pytest.approx(B * ENVS / (d["ms_per_step"] * 1e-3), rel=1e-9)
    for leg in ("cpu_baseline", "chunk_200", "per_step_launch", "dropin", "a2c_training", "scale_16x_envs"):
        assert d[leg] is None, leg
    assert sorted(os.listdir(out_dir)) == sorted(k + ".npy" for k in NAMES)
    assert sum(a.nbytes for a in arrays.values()) == d["dump_outputs"]["bytes"] <= 64 * 10**6
    for k, dt in NAMES.items():
        assert arrays[k].dtype == dt, k


def test_two_runs_dump_the_same_arrays(runs):
    for k in NAMES:
        assert runs[0][1][k].tobytes() == runs[1][1][k].tobytes(), k


def test_dump_is_the_oracle_trajectory_of_the_last_step(runs):
    from oracle import oracle as O
    d, arrays, _ = runs[0]
    total = (WARMUP + STEPS) * B
    rec, _, _ = O.rollout(ENVS, total, seeds=np.arange(ENVS), gid0=0, num_orders=30, action_seed=1234, policy=0)
    # the last launch holds the last 128 env-steps; the last bench step is its last B rows
    rows = np.asarray(d["dump_outputs"]["rows_of_last_launch"])
    assert rows.tolist() == list(range(128 - B, 128)) and d["dump_outputs"]["envs"] == ENVS
    steps = total - 128 + rows
    for k in ("obs_i32", "masks", "rewards"):
        want = np.asarray(rec[k])[steps].transpose(0, 2, 1)          # oracle [T, N, F] -> dump [T, F, N]
        assert np.array_equal(arrays[k], want.astype(arrays[k].dtype)), k
    for k in ("term", "trunc"):
        assert np.array_equal(arrays[k], np.asarray(rec[k])[steps].astype(np.float32)), k


def test_a2c_workload_dumps_the_last_batch(tmp_path):
    """--workload a2c: the parameters after the last timed update, the loss history and the last
    batch's rewards (every step and env of this small batch)."""
    T = 32
    d = _bench(tmp_path, "--workload", "a2c", "--steps", "2", "--warmup", "1", "--batch-size", str(T))
    assert d["steps"] == 2 and d["ms_per_step"] == d["a2c"]["ms_per_batch"] > 0
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["actor_params", "critic_loss_history", "critic_params", "rewards"] == sorted(
        d["a2c"]["dump_outputs"]["arrays"])
    assert got["rewards"].shape == (T, 8, ENVS) and got["rewards"].dtype == np.float64
    assert got["actor_params"].dtype == got["critic_params"].dtype == np.float32
    assert np.isfinite(got["actor_params"]).all() and np.isfinite(got["critic_params"]).all()
    assert got["critic_loss_history"][-1] == d["a2c"]["critic_loss_last"]
    assert sum(a.nbytes for a in got.values()) == d["a2c"]["dump_outputs"]["bytes"] <= 64 * 10**6
