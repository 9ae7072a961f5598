"""k_step_ag's E3 wave runs the pickup station two steps ahead, before the AGV of the step between
has acted, and composes the AGV's result into it for P (csrc/fjsp_env.h: pickup_compose).  A lane
AM reset, and a launch's first step, run their pickup behind AM's post as before.  Launches shorter than the
look-ahead, launch boundaries right before, at and after the truncation reset, resets at different
steps per lane (1 order; staggered episodes) and a tray pool that is empty most of the time: every lean output of
every step must be the oracle's, and so must 20 more steps from the state left behind (snapshot ->
restore into a fresh handle); no hand-off wait may give up, and a stalled owner wave still makes
the others give up."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import parity_util as P  # noqa: E402

AG = "k_step_ag<lds,predraw>"
LEAN = ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards", "term", "trunc", "status")
# 450 steps in launches of 1, 2, 3, 7, 201 and the rest, the rest cut right before, at and after the
# second truncation reset (episodes of 201 steps: AM resets at the top of steps 201 and 402)
LAUNCHES = (1, 2, 3, 7, 201, 186, 1, 1, 1, 47)
TAIL = 20
SEED = 23
N = 48   # 3 workgroups at 16 envs each, 1 + a half at 32, a partial one at 64
SPIN_TIMEOUT = 0x80
# Under uniform-random actions 2 orders are not completed within an episode (the oracle: no env of
# these terminates), so the resets of the first three cases are the lockstep truncations; one order
# is completed now and then, and the staggered test below truncates every lane at its own step.
CASES = {"2 orders": (2, {}), "30 orders": (30, {}), "30 orders, 3 trays": (30, dict(num_trays=3)), "1 order": (1, {})}


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util
    return gpu_util


def _seeds(n):
    return np.arange(n) * 5 + 11


@functools.lru_cache(maxsize=None)
def _oracle(case):
    num_orders, cfg = CASES[case]
    rec, _, _ = O.rollout(N, sum(LAUNCHES) + TAIL, seeds=_seeds(N), num_orders=num_orders, action_seed=SEED, policy=0, **cfg)
    rec.setflags(write=False)
    return rec


def _pool_empty(masks):
    """Share of the env-steps whose pickup masks (fields 1 LOAD, 2 SIGNAL) are both 0."""
    return float(((masks[:, :, 1] == 0) & (masks[:, :, 2] == 0)).mean())


def _mixed(ended):
    """A step after which some, not all, of the first 16 envs (one wave at every size) were reset."""
    k = ended[:, :16].sum(axis=1)
    return bool(((k > 0) & (k < 16)).any())


def _env(G, ag_envs, cfg, **opts):
    env = G.make_env(N, **cfg)
    L = G.native.lib()
    G.native.check(L.fjsp_set_option(env.handle, b"ag_envs", ag_envs))
    for k, v in opts.items():
        G.native.check(L.fjsp_set_option(env.handle, k.encode(), v))
    return env


def _launches(G, env, launches, t0=0):
    parts, t = [], t0
    for k in launches:
        parts.append(G.to_np(env.rollout(k, action_seed=SEED, step0=t, policy="random")))
        assert env.last_kernel() == AG
        t += k
    return {key: np.concatenate([p[key] for p in parts]) for key in LEAN}


@pytest.mark.parametrize("ag_envs", [16, 32, 64])
@pytest.mark.parametrize("case", list(CASES))
def test_against_the_oracle(G, case, ag_envs):
    num_orders, cfg = CASES[case]
    rec = _oracle(case)
    env = _env(G, ag_envs, cfg)
    env.reset(seeds=torch.from_numpy(_seeds(N)), num_orders=num_orders)
    got = _launches(G, env, LAUNCHES)
    env2 = _env(G, ag_envs, cfg)
    env2.restore(env.snapshot())
    tail = _launches(G, env2, (TAIL,), t0=sum(LAUNCHES))
    got = {k: np.concatenate([got[k], tail[k]]) for k in LEAN}
    for k in ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards"):
        assert P.bits_equal(got[k], rec[k]), k
    for k in ("term", "trunc"):
        assert np.array_equal(got[k], rec[k]), k
    P.status_parity(got["status"], rec, what="k_step_ag", got_ended=got["term"] | got["trunc"])
    assert env.faults() == 0 and env2.faults() == 0 and not (got["status"] & SPIN_TIMEOUT).any()
    ended = got["term"].astype(bool) | got["trunc"].astype(bool)
    assert ended.sum() >= 2 * N   # the truncations at least
    if num_orders == 1:   # an order completes: a step with lanes AM reset and others in one wave
        assert got["term"].sum() > 0 and _mixed(ended)
    if "num_trays" in cfg:   # no tray on the station and LOAD masked with orders at hand: the pool is empty
        assert _pool_empty(got["masks"]) > 0.5


@pytest.mark.parametrize("ag_envs", [16, 32, 64])
def test_staggered_episodes_against_k_step_pipe(G, ag_envs):
    """Masked resets between the launches start the lanes' episodes at different steps, so the
    37-step truncations meet fresh and other lanes in one wave, in launches of every small size:
    the bytes of k_step_pipe (which runs every agent in place)."""
    outs = []
    for opts in (dict(ag_envs=ag_envs), dict(agents=0)):
        env = G.make_env(N, max_episode_steps=37)
        for k, v in opts.items():
            G.native.check(G.native.lib().fjsp_set_option(env.handle, k.encode(), v))
        env.reset(seeds=torch.from_numpy(_seeds(N)), num_orders=3)
        seq, t = [], 0
        for i, k in enumerate((13, 29, 8, 50)):
            seq.append(G.to_np(env.rollout(k, action_seed=SEED, step0=t, policy="random")))
            t += k
            mask = ((torch.arange(N) % (i + 2)) == 0).to(torch.uint8).to(env.device)
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


def test_a_stalled_owner_wave_still_gives_up(G):
    """Workgroup 0's AM sleeps past the smallest bound of the other waves' waits (option
    "test_stall"): they give up, the launch ends, the fault word and the envs' status say so."""
    env = _env(G, 16, {}, spin_cap=256, test_stall=64)
    env.reset(seeds=torch.from_numpy(_seeds(N)), num_orders=30)
    st = _launches(G, env, (64,))["status"]
    assert env.faults() & 1
    flagged = (st[-1] & SPIN_TIMEOUT) != 0
    assert flagged[0] and ((st[-1][flagged] & 0x81) == 0x81).all()
