"""Output addressing of the multi-wave step kernels.  k_step_ag's four emit roles read the output
pointers and the env count as scalar kernel arguments, each role its own, and store through a scalar
base + the lane's offset; k_step_pipe's emit waves are checked the same way.  Every output of
`Buffers` is the contiguous middle of a slab
with two more rows before and after it, pre-filled with a sentinel byte: after the launches the
guard rows are untouched (a wrong base or field stride that lands inside the allocation faults
nowhere) and every output equals the oracle's bit for bit.  Three launches of 70 steps with `step0`
carried on cross a launch start twice and the 201-step truncation."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import parity_util as P  # noqa: E402

AG = "k_step_ag<lds,predraw>"
CHUNK, LAUNCHES = 70, 3
STEPS = CHUNK * LAUNCHES
SEED = 17
GUARD, SENTINEL = 2, 0xA5
LEAN = ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards", "term", "trunc", "status")
ORACLE_POLICY = {"random": 0, "masked": 1, "heuristic": 3}


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util
    return gpu_util


def _seeds(n):
    return np.arange(n) * 5 + 3


@functools.lru_cache(maxsize=None)
def _oracle(n, num_orders, policy):
    rec, _, _ = O.rollout(n, STEPS, seeds=_seeds(n), num_orders=num_orders, action_seed=SEED,
                          policy=ORACLE_POLICY[policy])
    rec.setflags(write=False)
    return rec


class Guarded:
    """Buffers(CHUNK, n) whose outputs are rows [GUARD, GUARD + CHUNK) of sentinel-filled slabs."""

    def __init__(self, G, n, device, absent=()):
        self.buf = G.vec_env.Buffers(CHUNK, n, device, infos=False)
        self.slabs = {}
        for key in LEAN:
            t = getattr(self.buf, key)
            if key in absent:
                setattr(self.buf, key, None)
                continue
            slab = torch.empty((CHUNK + 2 * GUARD,) + tuple(t.shape[1:]), dtype=t.dtype, device=device)
            slab.view(torch.uint8).fill_(SENTINEL)
            mid = slab[GUARD:GUARD + CHUNK]
            assert mid.is_contiguous() and mid.shape == t.shape
            setattr(self.buf, key, mid)
            self.slabs[key] = slab

    def refill(self):
        for slab in self.slabs.values():
            slab[GUARD:GUARD + CHUNK].view(torch.uint8).fill_(SENTINEL)

    def check_guards(self, what):
        for key, slab in self.slabs.items():
            for part in (slab[:GUARD], slab[GUARD + CHUNK:]):
                b = part.contiguous().view(torch.uint8)
                assert bool((b == SENTINEL).all()), (what, key, "guard rows written")


def _run(G, n, num_orders, policy, opts, kernel, absent=()):
    env = G.make_env(n)
    for k, v in opts.items():
        G.native.check(G.native.lib().fjsp_set_option(env.handle, k.encode(), v))
    env.reset(seeds=torch.from_numpy(_seeds(n)), num_orders=num_orders)
    g = Guarded(G, n, env.device, absent)
    parts = []
    for i in range(LAUNCHES):
        g.refill()
        env.rollout(CHUNK, action_seed=SEED, step0=i * CHUNK, policy=policy, buffers=g.buf)
        torch.cuda.synchronize()
        assert kernel in env.last_kernel(), env.last_kernel()
        g.check_guards((n, num_orders, policy, i))
        parts.append(G.to_np(g.buf))
    assert env.faults() == 0
    got = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    rec = _oracle(n, num_orders, policy)
    assert set(got) == set(LEAN) - set(absent)
    for key in ("obs_i32", "obs_i8", "obs_f32", "masks", "rewards"):
        if key in got:
            assert P.bits_equal(got[key], rec[key]), key
    for key in ("term", "trunc"):
        if key in got:
            assert np.array_equal(got[key], rec[key]), key
    if "status" in got:
        ended = (got["term"] | got["trunc"]) if "term" in got else (rec["term"] | rec["trunc"])
        P.status_parity(got["status"], rec, what=kernel, got_ended=ended)
    if "trunc" in got and policy == "random":
        assert got["trunc"].sum() >= n            # the 201-step truncation
    return got


# 40 envs: three workgroups of 16, the last with 8 lanes; 128: 8 workgroups, the workgroup remap
# over the XCDs is active; 136: 17 workgroups, the remap is off; 70 envs at 32 and 64 per workgroup
SHAPES = [(40, 16), (128, 16), (136, 16), (70, 32), (70, 64)]


@pytest.mark.parametrize("num_orders", [2, 30])
@pytest.mark.parametrize("n,ag_envs", SHAPES)
def test_agents_guarded(G, n, ag_envs, num_orders):
    """k_step_ag, uniform-random actions: every lean output bit-equal to the oracle's, guards untouched."""
    _run(G, n, num_orders, "random", dict(ag_envs=ag_envs), AG)


ABSENT = [("rewards", "masks"), ("obs_i32", "obs_f32"), ("obs_i8", "term", "trunc", "status")]


@pytest.mark.parametrize("absent", ABSENT, ids=["-".join(a) for a in ABSENT])
def test_agents_absent_outputs(G, absent):
    """Every emit role loses at least one output (E0 rewards, E0 / E2 / E3 masks; E1 both of its
    outputs; E2 all but its masks): the others stay bit-equal, the guards untouched."""
    _run(G, 40, 30, "random", dict(ag_envs=16), AG, absent=absent)


@pytest.mark.parametrize("policy,num_orders", [("masked", 30), ("heuristic", 5)])
def test_pipe_guarded(G, policy, num_orders):
    """k_step_pipe (state-dependent actions): 70 envs, two workgroups, the last with 6 lanes."""
    _run(G, 70, num_orders, policy, {}, "k_step_pipe")
