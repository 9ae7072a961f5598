"""k_step_ag's P wave resolves the AGV's step in two halves (csrc/fjsp_env.h: agv_pre before the
other agents' hand-offs arrive, agv_fin after them).  Small rollouts through `rollout` against the
oracle: three launches of 150 steps cross the 201-step truncation reset and start three times with
the step AM runs itself; 40 envs at 16 per workgroup are three workgroups, the last with 8 valid
lanes; 2 orders per episode keep the lists short (the paths where a list's front or its successor
appears between the halves), 30 keep them long."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import parity_util as P  # noqa: E402

AG = "k_step_ag<lds,predraw>"
CHUNKS = (150, 150, 150)
TAIL = 3
SEED = 13


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util
    return gpu_util


def _seeds(n):
    return np.arange(n) * 7 + 5


@functools.lru_cache(maxsize=None)
def _oracle(n, num_orders):
    rec, _, _ = O.rollout(n, sum(CHUNKS) + TAIL, seeds=_seeds(n), num_orders=num_orders, action_seed=SEED, policy=0)
    rec.setflags(write=False)
    return rec


def _check(G, n, num_orders, ag_envs):
    env = G.make_env(n)
    if ag_envs:
        G.native.check(G.native.lib().fjsp_set_option(env.handle, b"ag_envs", ag_envs))
    env.reset(seeds=torch.from_numpy(_seeds(n)), num_orders=num_orders)
    parts, t = [], 0
    for k in CHUNKS:
        parts.append(G.to_np(env.rollout(k, action_seed=SEED, step0=t, policy="random")))
        assert env.last_kernel() == AG
        t += k
    got = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    # the state left behind: full-output steps of another kernel from it
    tail = G.to_np(env.rollout(TAIL, action_seed=SEED, step0=t, policy="random", infos=True))
    assert env.last_kernel() != AG
    rec = _oracle(n, num_orders)
    head, last = rec[:t], rec[t:]
    for key in ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards"):
        assert P.bits_equal(got[key], head[key]), key
    for key in ("term", "trunc"):
        assert np.array_equal(got[key], head[key]), key
    P.status_parity(got["status"], head, what="k_step_ag", got_ended=got["term"] | got["trunc"])
    assert got["trunc"].sum() >= n            # the 201-step truncation
    for key in ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards", "results"):
        assert P.bits_equal(tail[key], last[key]), ("state after the launches", key)
    for key in ("term", "trunc", "orders_completed", "packaged"):
        assert np.array_equal(tail[key], last[key]), ("state after the launches", key)


@pytest.mark.parametrize("num_orders", [2, 30])
def test_three_workgroups_last_partial(G, num_orders):
    """40 envs, 16 per workgroup: every lean output and the state left behind equal the oracle's."""
    _check(G, 40, num_orders, 0)


@pytest.mark.parametrize("ag_envs", [32, 64])
@pytest.mark.parametrize("num_orders", [2, 30])
def test_other_envs_per_workgroup(G, num_orders, ag_envs):
    """70 envs at 32 and 64 envs per workgroup (partial last workgroups of 6 lanes)."""
    _check(G, 70, num_orders, ag_envs)
