"""k_step_ag's pre-draw wave draws the next order table in slices (csrc/fjsp_predraw.h): a load, a
refill and a consume that fall in different steps, alternating by the step's parity at 16 envs
per workgroup.  Resets before, at and after the table's readiness, launch boundaries on every slice
phase and inside the row-copy stagger: the lean outputs must be the bytes of the same rollout
without the pre-draw (k_step_pipe<lds,2emit>) and of the oracle, the MT streams must end equal,
and after a launch long enough every env's table must be ready (without that condition a pre-draw
that never finishes would pass every byte comparison through the inline reset)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import parity_util as P  # noqa: E402

AG = "k_step_ag<lds,predraw>"
PIPE = "k_step_pipe<lds,2emit>"
LEAN = ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards", "term", "trunc", "status")
LAUNCHES = (1, 2, 3, 5, 7, 11, 13, 17, 150, 41, 200)   # 450 steps
SEED = 21
N = 40   # partial workgroups at 16, 32 and 64 envs per workgroup
PGW = 30   # the pre-draw record's row of the state words (fjsp_stepdev.h)
SPIN_TIMEOUT = 0x80


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util
    return gpu_util


def _seeds(n):
    return np.arange(n) * 3 + 17


def _env(G, n, ag_envs, **cfg):
    """ag_envs = 0: the rollout without the pre-draw wave."""
    env = G.make_env(n, **cfg)
    L = G.native.lib()
    if ag_envs:
        G.native.check(L.fjsp_set_option(env.handle, b"ag_envs", ag_envs))
    else:
        G.native.check(L.fjsp_set_option(env.handle, b"predraw", 0))
    return env


def _launches(G, env, name, launches=LAUNCHES, t0=0):
    parts, t = [], t0
    for k in launches:
        parts.append(G.to_np(env.rollout(k, action_seed=SEED, step0=t, policy="random")))
        assert env.last_kernel() == name
        t += k
    return {key: np.concatenate([p[key] for p in parts]) for key in LEAN}


def _freeze(d):
    for v in d.values():
        v.setflags(write=False)
    return d


_G = []   # gpu_util for the cached references


@functools.lru_cache(maxsize=None)
def _plain(n, num_orders, mes):
    """The rollout without the pre-draw, its MT streams, and the oracle's records."""
    G = _G[0]
    env = _env(G, n, 0, max_episode_steps=mes)
    env.reset(seeds=torch.from_numpy(_seeds(n)), num_orders=num_orders)
    out = _freeze(_launches(G, env, PIPE))
    mts = {e: env.mt_get(e) for e in sorted({0, min(15, n - 1), min(16, n - 1), n - 1})}
    rec, _, _ = O.rollout(n, sum(LAUNCHES), seeds=_seeds(n), num_orders=num_orders, action_seed=SEED, policy=0,
                          max_episode_steps=mes)
    rec.setflags(write=False)
    return out, mts, rec


def _check(G, n, ag_envs, num_orders, mes):
    if not _G:
        _G.append(G)
    want, mts, rec = _plain(n, num_orders, mes)
    env = _env(G, n, ag_envs, max_episode_steps=mes)
    env.reset(seeds=torch.from_numpy(_seeds(n)), num_orders=num_orders)
    got = _launches(G, env, AG)
    for k in LEAN:
        assert P.bits_equal(got[k], want[k]), k
    for k in ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards"):
        assert P.bits_equal(got[k], rec[k]), ("oracle", k)
    for k in ("term", "trunc"):
        assert np.array_equal(got[k], rec[k]), ("oracle", k)
    P.status_parity(got["status"], rec, what="k_step_ag", got_ended=got["term"] | got["trunc"])
    assert env.faults() == 0 and not (got["status"] & SPIN_TIMEOUT).any()
    assert got["trunc"].sum() + got["term"].sum() >= n * (sum(LAUNCHES) // (mes + 1) - 1)   # the resets happened
    for e, (key, pos) in mts.items():
        k2, p2 = env.mt_get(e)
        assert p2 == pos and np.array_equal(k2, key), ("mt", e)


@pytest.mark.parametrize("ag_envs", [16, 32, 64])
@pytest.mark.parametrize("mes", range(4, 41))
def test_short_episodes_reset_before_at_and_after_readiness(G, mes, ag_envs):
    """3 orders, episodes of 5 .. 41 steps: the reset meets the lane idle, copying, in every slice
    and ready."""
    _check(G, N, ag_envs, 3, mes)


@pytest.mark.parametrize("ag_envs", [16, 32, 64])
@pytest.mark.parametrize("num_orders,mes", [(30, 20), (30, 60), (30, 128), (30, 200), (64, 200)])
def test_long_tables(G, num_orders, mes, ag_envs):
    _check(G, N, ag_envs, num_orders, mes)


def test_one_env(G):
    _check(G, 1, 16, 30, 60)


@pytest.mark.parametrize("ag_envs", [16, 32, 64])
def test_staggered_masked_resets_between_launches(G, ag_envs):
    """Lanes whose episodes start at different steps (masked resets between the launches)."""
    n = N
    outs = []
    for epw, name in ((ag_envs, AG), (0, PIPE)):
        env = _env(G, n, epw, max_episode_steps=37)
        env.reset(seeds=torch.from_numpy(_seeds(n)), num_orders=3)
        seq, t = [], 0
        for i, k in enumerate((13, 29, 8, 50)):
            seq.append(_launches(G, env, name, (k,), t0=t))
            t += k
            mask = ((torch.arange(n) % (i + 2)) == 0).to(torch.uint8).to(env.device)
            env.reset(env_mask=mask, num_orders=3)
        seq.append(_launches(G, env, name, (90, 45, 120), t0=t))
        outs.append((seq, env))
    (a, ea), (b, eb) = outs
    for i, (x, y) in enumerate(zip(a, b)):
        for k in LEAN:
            assert P.bits_equal(x[k], y[k]), (i, k)
    assert ea.faults() == 0 and not any((x["status"] & SPIN_TIMEOUT).any() for x in a)
    for e in (0, 15, 16, n - 1):
        (ka, pa), (kb, pb) = ea.mt_get(e), eb.mt_get(e)
        assert pa == pb and np.array_equal(ka, kb), e


@pytest.mark.parametrize("ag_envs", [16, 32, 64])
@pytest.mark.parametrize("num_orders,steps", [(30, 128), (30, 190), (64, 190)])
def test_the_table_is_ready(G, num_orders, steps, ag_envs):
    """One launch from a fresh reset: the pre-draw record of every env (bit 0 ready, bits 24-30
    the order count) says the table was finished, so the reset that follows is a table copy."""
    env = _env(G, N, ag_envs)
    env.reset(seeds=torch.from_numpy(_seeds(N)), num_orders=num_orders)
    env.rollout(steps, action_seed=SEED, step0=0, policy="random")
    assert env.last_kernel() == AG and env.faults() == 0
    words = env.snapshot().cpu().numpy().view(np.uint32)
    pg = words[PGW * N:(PGW + 1) * N]
    assert (pg & 1).all(), np.flatnonzero((pg & 1) == 0)
    assert (((pg >> 24) & 0x7F) == num_orders).all()
