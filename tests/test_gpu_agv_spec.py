"""k_step_ag's P wave runs the first half of the AGV's step (csrc/fjsp_env.h: agv_pre) on the words
of its own last AGV, unless AM reset the lane in this step: then on AM's post.  agv_pre is not
pure: a DROP stores `snext[carry] = NIL` into the slot table, and on a lane AM resets the stale
`carry` names a slot of the dead episode that AM's pickup may be linking in the same step.  These
cases pin that hazard for any schedule of agv_pre (a version that started it before the reset
decision was built and measured, profiles/machine_lanes/; it is not kept): (a) short episodes
that end with the AGV carrying a tray and a DROP drawn for the next step, against the oracle;
(b) staggered episodes, fresh and other lanes in one wave, launches of every small size, against
k_step_pipe (which runs every agent in place)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import parity_util as P  # noqa: E402

AG = "k_step_ag<lds,predraw>"
LEAN = ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards", "term", "trunc", "status")
SEED = 17
N = 40   # 16 per workgroup: three workgroups, the last with 8 lanes
EPISODE = 37
LAUNCHES = (70, 70, 70)
SPIN_TIMEOUT = 0x80


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util
    return gpu_util


def _seeds(n):
    return np.arange(n) * 5 + 3


@functools.lru_cache(maxsize=None)
def _oracle():
    rec, _, _ = O.rollout(N, sum(LAUNCHES), seeds=_seeds(N), num_orders=3, action_seed=SEED, policy=0,
                          max_episode_steps=EPISODE)
    rec.setflags(write=False)
    return rec


def hazards(rec):
    """Episode ends whose last record has the AGV carrying a tray (obs_i32[9]) and whose next
    step's AGV action is DROP (7): the stale agv_pre of that step would push the dead episode's
    carried slot."""
    ended = rec["term"].astype(bool) | rec["trunc"].astype(bool)
    count = 0
    for t, e in zip(*np.nonzero(ended[:-1])):
        if rec["obs_i32"][t, e, 9] == 1 and O.actions(SEED, int(e), int(t) + 1)[1] == 7:
            count += 1
    return count


def _mixed(ended):
    """A step after which some, not all, of the first 16 envs (one wave at every size) were reset."""
    k = ended[:, :16].sum(axis=1)
    return bool(((k > 0) & (k < 16)).any())


@pytest.mark.parametrize("ag_envs", [16, 32, 64])
def test_episodes_end_carrying_with_a_drop_next(G, ag_envs):
    rec = _oracle()
    n_hazards = hazards(rec)
    print("episode ends with the AGV carrying and a DROP next:", n_hazards)
    assert n_hazards > 0
    env = G.make_env(N, max_episode_steps=EPISODE)
    G.native.check(G.native.lib().fjsp_set_option(env.handle, b"ag_envs", ag_envs))
    env.reset(seeds=torch.from_numpy(_seeds(N)), num_orders=3)
    parts, t = [], 0
    for k in LAUNCHES:
        parts.append(G.to_np(env.rollout(k, action_seed=SEED, step0=t, policy="random")))
        assert env.last_kernel() == AG
        t += k
    got = {key: np.concatenate([p[key] for p in parts]) for key in LEAN}
    for key in ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards"):
        assert P.bits_equal(got[key], rec[key]), key
    for key in ("term", "trunc"):
        assert np.array_equal(got[key], rec[key]), key
    P.status_parity(got["status"], rec, what="k_step_ag", got_ended=got["term"] | got["trunc"])
    assert env.faults() == 0 and not (got["status"] & SPIN_TIMEOUT).any()


@pytest.mark.parametrize("ag_envs", [16, 32, 64])
def test_staggered_episodes_against_k_step_pipe(G, ag_envs):
    """Masked resets between the launches start the lanes' episodes at different steps, so the
    37-step truncations meet fresh and other lanes in one wave; 3 trays keep the AGV's lists short."""
    n, outs = 48, []
    seeds = torch.from_numpy(np.arange(n) * 5 + 11)
    for opts in (dict(ag_envs=ag_envs), dict(agents=0)):
        env = G.make_env(n, max_episode_steps=EPISODE, num_trays=3)
        for k, v in opts.items():
            G.native.check(G.native.lib().fjsp_set_option(env.handle, k.encode(), v))
        env.reset(seeds=seeds, num_orders=3)
        seq, t = [], 0
        for i, k in enumerate((13, 29, 8, 50)):
            seq.append(G.to_np(env.rollout(k, action_seed=SEED, step0=t, policy="random")))
            t += k
            mask = ((torch.arange(n) % (i + 2)) == 0).to(torch.uint8).to(env.device)
            env.reset(env_mask=mask, num_orders=3)
        for k in (1, 2, 3, 7, 90, 45):
            seq.append(G.to_np(env.rollout(k, action_seed=SEED, step0=t, policy="random")))
            t += k
        assert env.last_kernel() == (AG if "ag_envs" in opts else "k_step_pipe<lds,2emit,predraw>"), env.last_kernel()
        assert env.faults() == 0
        outs.append({key: np.concatenate([p[key] for p in seq]) for key in LEAN})
    a, b = outs
    for k in LEAN:
        assert P.bits_equal(a[k], b[k]), k
    assert not (a["status"] & SPIN_TIMEOUT).any()
    assert _mixed(a["trunc"].astype(bool))
