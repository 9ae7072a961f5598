"""k_step_ag's AM wave on lane groups: with 16 / 32 envs per workgroup the two machines of an env
run on the wave's lane groups 0 and 1 (csrc/fjsp_env.h, mach_lane_*); group 1 keeps machine 1's
lists, its word and its status bits, which join the env's where the status is emitted and stored.

Uniform-random play from a reset never has both machines act in one step (the oracle: 0 such
steps of 40 and 70 envs x 210 steps at 1 / 2 / 30 orders), so every case starts from a warm-up of
explicit actions (the heuristic policy's, the machines idle: both queues fill to 3), stepped one
launch per step; then three launches of 70 random steps on k_step_ag into guarded slabs
(tests/test_gpu_emit_stores.py), every output bit-equal to the oracle's replay of the same action
stream.  The oracle's record must itself show both machines starting in one step, both finishing a
tray in one step and ST_OVERWRITE (a START granted onto a machine that still holds a tray, which
stays inside the comparison), so a case cannot pass on nothing.  A last case puts every launch
boundary on machines with work: the first step of a launch loads group 1's words and hands machine
1's lists over, the last stores them."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import parity_util as P  # noqa: E402
from tests.test_gpu_emit_stores import AG, CHUNK, LAUNCHES, STEPS, Guarded  # noqa: E402

SEED = 17
ST_OVERWRITE = 0x20


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util
    return gpu_util


def _seeds(n):
    return np.arange(n) * 5 + 3


@functools.lru_cache(maxsize=None)
def _oracle(n, num_orders, warm):
    """(actions [warm + STEPS, n, 8], the oracle's record of them): warm steps of the heuristic's
    actions with the machines idle, then the counter RNG's uniform actions of step t."""
    seeds = _seeds(n)
    acts = np.zeros((warm + STEPS, n, 8), np.uint8)
    for e in range(n):
        env = O.OracleEnv()
        env.reset(seed=int(seeds[e]), num_orders=num_orders)
        for t in range(warm):
            a = env.heuristic()
            a[2:4] = 0
            acts[t, e] = a
            r = env.step(a)
            assert not (r["term"] or r["trunc"]), "the warm-up stays inside the first episode"
        for t in range(warm, warm + STEPS):
            acts[t, e] = O.actions(SEED, e, t)
    rec, _, _ = O.rollout(n, warm + STEPS, seeds=seeds, num_orders=num_orders, actions_in=acts)
    rec.setflags(write=False)
    acts.setflags(write=False)
    return acts, rec


def events(rec, warm):
    """From the record of the random phase: steps in which both machines START, one STARTs and the
    other SIGNALs, both SIGNAL (result words, bits 2 / 4), both finish a tray (busy 1 -> 0 inside an
    episode); the share of env-steps with ST_OVERWRITE; envs that truncate."""
    res = rec["results"][warm:, :, 2:4].astype(np.int64)
    go, sig = (res & 2) != 0, (res & 4) != 0
    i8 = rec["obs_i8"][warm - 1:]
    same = ~(rec["term"] | rec["trunc"]).astype(bool)[warm - 1:-1]
    busy = i8[:, :, 0:4:2].astype(int)
    fin = (busy[:-1] == 1) & (busy[1:] == 0) & same[:, :, None]
    return dict(both_start=int(go.all(-1).sum()), start_signal=int(((go[..., 0] & sig[..., 1]) | (sig[..., 0] & go[..., 1])).sum()),
                both_signal=int(sig.all(-1).sum()), both_finish=int(fin.all(-1).sum()),
                overwrite=float(((rec["status"][warm:] & ST_OVERWRITE) != 0).mean()),
                truncated=int((rec["trunc"][warm:].sum(0) > 0).sum()))


def _run(G, n, ag_envs, num_orders, warm, launches):
    acts, rec = _oracle(n, num_orders, warm)
    ev = events(rec, warm)
    print((n, ag_envs, num_orders), ev)
    assert ev["both_start"] > 0 and ev["both_finish"] > 0 and ev["overwrite"] > 0, ev
    env = G.make_env(n)
    G.native.check(G.native.lib().fjsp_set_option(env.handle, b"ag_envs", ag_envs))
    env.reset(seeds=torch.from_numpy(_seeds(n)), num_orders=num_orders)
    dev_acts = torch.from_numpy(np.ascontiguousarray(acts[:warm].transpose(0, 2, 1))).to(env.device)
    for t in range(warm):
        env.step(dev_acts[t])
    g = Guarded(G, n, env.device)
    parts, t = [], warm
    for i, k in enumerate(launches):
        g.refill()
        env.rollout(k, action_seed=SEED, step0=t, policy="random", buffers=g.buf)
        torch.cuda.synchronize()
        assert AG in env.last_kernel(), env.last_kernel()
        g.check_guards((n, ag_envs, num_orders, i))
        parts.append({key: v[:k] for key, v in G.to_np(g.buf).items()})
        t += k
    assert env.faults() == 0
    got = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    want = rec[warm:t]
    P.status_parity(got["status"], want, what=AG, got_ended=got["term"] | got["trunc"])
    assert not (got["status"] & 1).any()          # nothing diverged: every env-step is compared
    assert ((got["status"] & ST_OVERWRITE) != 0).any()
    for key in ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards"):
        assert P.bits_equal(got[key], want[key]), key
    for key in ("term", "trunc"):   # (status_parity compares ST_OVERWRITE bit by bit)
        assert np.array_equal(got[key], want[key]), key
    return got


# 40 envs at 16 per workgroup: the last workgroup has 8 lanes per group; 70 at 32 and 64 (one lane
# per env: the sequence)
CASES = [(40, 16, 30, 100), (40, 16, 2, 100), (70, 32, 30, 100), (70, 64, 30, 100)]


@pytest.mark.parametrize("n,ag_envs,num_orders,warm", CASES)
def test_machine_lanes_guarded(G, n, ag_envs, num_orders, warm):
    got = _run(G, n, ag_envs, num_orders, warm, (CHUNK,) * LAUNCHES)
    assert (got["trunc"].sum(0) > 0).all()        # every lane truncates in the random phase


def test_launch_boundaries_on_machines_with_work(G):
    """Launches of 1, 2, 3, 7 and 57 steps right after the warm-up, 16 envs per workgroup: every
    boundary loads group 1's words at its first step and stores them after its last."""
    _run(G, 40, 16, 30, 100, (1, 2, 3, 7, 57))
