"""k_step_ag's packaging wave on lane groups: with 16 / 32 envs per workgroup the four stations of
an env run on the wave's four / two lane groups (csrc/fjsp_env.h, pack_lane_*), their counts summed
and their status bits ORed across the groups once per step.

Uniform-random actions almost never leave two stations with work at once, so every case starts
from a warm-up of explicit actions (the heuristic policy's, the packaging stations idle: their
queues fill), stepped one launch per step; then three launches of 70 random steps on k_step_ag into
guarded slabs (tests/test_gpu_emit_stores.py), every output bit-equal to the oracle's replay of
the same action stream.  The oracle's record must itself show packaging completions at two
stations in one step and drops to more than one station, so a case cannot pass on nothing."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import parity_util as P  # noqa: E402
from tests.test_gpu_emit_stores import AG, CHUNK, LAUNCHES, STEPS, Guarded  # noqa: E402

SEED = 17
SMALL_PKG = dict(storage_capacity=2, packaging_capacity=3)   # of test_agents_configs (8 orders)


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util
    return gpu_util


def _seeds(n):
    return np.arange(n) * 5 + 3


@functools.lru_cache(maxsize=None)
def _oracle(n, num_orders, small_pkg, warm):
    """(actions [warm + STEPS, n, 8], the oracle's record of them): warm steps of the heuristic's
    actions with the packaging stations idle, then the counter RNG's uniform actions of step t."""
    cfg = SMALL_PKG if small_pkg else {}
    seeds = _seeds(n)
    acts = np.zeros((warm + STEPS, n, 8), np.uint8)
    for e in range(n):
        env = O.OracleEnv(**cfg)
        env.reset(seed=int(seeds[e]), num_orders=num_orders)
        for t in range(warm):
            a = env.heuristic()
            a[4:8] = 0
            acts[t, e] = a
            r = env.step(a)
            assert not (r["term"] or r["trunc"]), "the warm-up stays inside the first episode"
        for t in range(warm, warm + STEPS):
            acts[t, e] = O.actions(SEED, e, t)
    rec, _, _ = O.rollout(n, warm + STEPS, seeds=seeds, num_orders=num_orders, actions_in=acts, **cfg)
    rec.setflags(write=False)
    acts.setflags(write=False)
    return acts, rec


def _flagged(rec):
    """Env-steps of the whole record that are out of the comparison: the oracle marks them as off
    the reference's normal path, or the reference raised earlier (the oracle zeroes that env's
    records from then on and never resets it; tests/parity_util.py, status_parity)."""
    st = np.asarray(rec["status"])
    raised = np.logical_or.accumulate((st & O.ST_EXCEPTION) != 0, axis=0)
    return ((st & (O.ST_EXCEPTION | O.ST_PKG_WAIT | O.ST_OBS_OVERFLOW)) != 0) | raised


def _events(rec, warm):
    """From the record of the random phase, comparable env-steps only: those in which two stations'
    batches completed (busy 1 -> 0 inside an episode), and per station those in which its queue
    grew (a drop)."""
    i8 = rec["obs_i8"][warm - 1:]
    same = ~(rec["term"] | rec["trunc"]).astype(bool)[warm - 1:-1] & ~_flagged(rec)[warm:]
    busy, queued = i8[:, :, 4:12:2].astype(int), i8[:, :, 5:12:2].astype(int)
    fin = (busy[:-1] == 1) & (busy[1:] == 0) & same[:, :, None]
    drops = ((queued[1:] > queued[:-1]) & same[:, :, None]).sum((0, 1))
    return int((fin.sum(-1) >= 2).sum()), drops


# 40 envs at 16 per workgroup: the last workgroup has 8 lanes per group; 70 at 32 and 64.  The
# small-capacity config (stations fill up; a START with more than 3 products queued leaves the
# comparison, as in test_agents_configs) after a shorter warm-up, so that a quarter of the env-steps
# and not nine tenths are flagged, at 16 per workgroup with 70 envs (the last workgroup has 6 lanes
# per group).
CASES = [(40, 16, 2, False, 100), (40, 16, 30, False, 100), (70, 32, 2, False, 100), (70, 32, 30, False, 100),
         (70, 64, 2, False, 100), (70, 64, 30, False, 100), (70, 16, 8, True, 40)]


@pytest.mark.parametrize("n,ag_envs,num_orders,small_pkg,warm", CASES)
def test_station_lanes_guarded(G, n, ag_envs, num_orders, small_pkg, warm):
    acts, rec = _oracle(n, num_orders, small_pkg, warm)
    simultaneous, drops = _events(rec, warm)
    assert simultaneous > 0 and (drops > 0).sum() >= 2, (simultaneous, drops)
    env = G.make_env(n, **(SMALL_PKG if small_pkg else {}))
    G.native.check(G.native.lib().fjsp_set_option(env.handle, b"ag_envs", ag_envs))
    env.reset(seeds=torch.from_numpy(_seeds(n)), num_orders=num_orders)
    dev_acts = torch.from_numpy(np.ascontiguousarray(acts[:warm].transpose(0, 2, 1))).to(env.device)
    for t in range(warm):
        env.step(dev_acts[t])
    g = Guarded(G, n, env.device)
    parts = []
    for i in range(LAUNCHES):
        g.refill()
        env.rollout(CHUNK, action_seed=SEED, step0=warm + i * CHUNK, policy="random", buffers=g.buf)
        torch.cuda.synchronize()
        assert AG in env.last_kernel(), env.last_kernel()
        g.check_guards((n, ag_envs, num_orders, i))
        parts.append(G.to_np(g.buf))
    assert env.faults() == 0
    got = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    want = rec[warm:]
    # which env-steps are flagged on either side is status_parity's to judge
    info = P.status_parity(got["status"], want, what=AG, got_ended=got["term"] | got["trunc"])
    ok = ~((got["status"] & 1).astype(bool) | _flagged(rec)[warm:])
    assert ok.all() if not small_pkg else 2 * ok.sum() > ok.size, info
    for key in ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards"):
        assert P.bits_equal(got[key][ok], want[key][ok]), key
    for key in ("term", "trunc"):
        assert np.array_equal(got[key][ok], want[key][ok]), key
    assert got["trunc"].sum() > 0            # the 201-step truncation falls in the random phase
