"""Every reward weight, on every selectable step path, against the oracle under the same weights.

The per-step f64 `rewards` are assembled in several places (env_advance with local_reward /
global_reward8 for k_step, the step server and k_step_many; k_step_pipe's emit wave from a packed
snapshot word; k_step_ag's emit waves from sixteen-bit halves written by two waves; k_policy_step
from a table that reaches LDS as raw 32-bit words; each kernel's own copy of the device table into
LDS), while every other comparison of rewards runs under the default weights, where several
mistakes change no bit: PICKUP_LOAD = MACHINE_START, PICKUP_TRAY_COMPLETE = MACHINE_COMPLETE,
PICKUP_IDLE = PACKAGING_IDLE, AGV_MOVE = TIME_PENALTY, and all but +-0.1 are small dyadic numbers.

Here each path runs configuration A (parity_util.STATUS_CFGS: defaults, 30 orders, action seed 13)
on the 200 envs of test_gpu_status.py (a partial last workgroup at 16, 32 and 64 envs per
workgroup) in launches of 60, 1, 139 and 60 steps under DISTINCT, GLOBAL_ONLY, SCALED and LOCAL_ONLY
(parity_util.REWARD_SETS), set between the launches; it is then snapshotted, restored into a fresh
handle on which DISTINCT is set, and run 20 steps more.  The dynamics do not depend on the weights,
so the expected rewards are one weighted oracle rollout per (policy, set), spliced by launch.
Asserted per path: rewards byte-equal to the spliced oracle rows on every env-step (configuration A
flags none), every other lean output and the status word byte-equal to the same path run under the
default weights (whose rewards equal the default oracle's), faults() == 0.  The oracle's weighted
rewards are themselves pinned to the reference (tests/test_oracle_golden.py::test_oracle_reward_weights),
the table and its readers exhaustively to utils/RewardModel.py (tests/test_hostsim_logic.py).

So that no test passes on nothing, each computes from the oracle's records alone on how many
env-steps every reward term is earned (parity_util.reward_term_counts), prints the counts and
asserts parity_util.REWARD_FLOOR = 10 for every term its policy can reach; the unreachable terms
are listed per policy (parity_util.REWARD_UNREACHABLE) and asserted to stay at zero.  The oracle
alone, 200 envs x 280 steps: random: smallest counts orders_completed 12, pkg_green.idle 13,
pkg_green.start 17; masked: orders_completed 22, pkg_green.start 37; heuristic: every term it
reaches > 500.

packaging_blue_2 earns nothing under any policy in configuration A: a tray goes to the first
station of its colour with a free Resource slot, which is packaging_blue_1 unless its slots are
all in use.  A bounded search with the oracle alone (scripts/search_status_cases.py blue2: masked actions, 200 envs x 280 steps: 432
configurations over packaging_capacity 1..3, tray_capacity 1..3, pt_packaging 250..2000, pt_small /
pt_big 10 or 60 / 120, episodes of 200 or 253 steps at action seed 13, then action seeds 0..399 on
the best six) found configuration F (parity_util.STATUS_CFGS: one Resource slot, trays of one
product, packaging runs of 100 steps, action seed 301): packaging_blue_2 starts / completes / idles
on 31 / 161 / 68 env-steps with nothing flagged (19 / 124 / 41 at action seed 13).  F runs on
fjsp_step, the step server and one k_step_pipe variant, under masked actions; there an order is
completed on one env-step only, so that term is exempt in F (parity_util.REWARD_EXEMPT_F) and A's
to cover.  Everywhere else packaging_blue_2's coverage is the exhaustive table test and the
comparison that both sides are zero.
"""
import functools
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import parity_util as P  # noqa: E402
from tests import test_gpu_status as S  # noqa: E402  (its helpers: _env, _host_steps' layout, _oracle, PIPES, ...)

N, CHUNKS, TAIL, STEPS = S.N, S.CHUNKS, S.TAIL, S.STEPS
SETS = ("DISTINCT", "GLOBAL_ONLY", "SCALED", "LOCAL_ONLY")      # one per launch of CHUNKS
TAIL_SET = "DISTINCT"                                           # set on the restored fresh handle
SEGMENTS = tuple(zip(np.cumsum((0,) + CHUNKS)[:-1].tolist(), np.cumsum(CHUNKS).tolist(), SETS)) + (
    (sum(CHUNKS), STEPS, TAIL_SET),)
OTHERS = tuple(k for k in S.LEAN if k != "rewards") + ("status",)
FLAGS = O.ST_EXCEPTION | O.ST_OBS_OVERFLOW | O.ST_PKG_WAIT

@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util
    return gpu_util


@functools.lru_cache(maxsize=None)
def _oracle_w(name, policy, sname):
    """rewards f64 [STEPS, N, 8] of the oracle's rollout of (configuration, policy) under the
    weight set sname (None: the defaults).  policy "host": the replay of _oracle_actions' stream."""
    c = P.STATUS_CFGS[name]
    w = None if sname is None else P.REWARD_SETS[sname]
    kw = dict(seeds=P.status_seeds(N), num_orders=c["num_orders"], weights=w, **c["cfg"])
    if policy == "host":
        acts, judge = S._oracle_actions(name)
        rec, _, _ = O.rollout(N, STEPS, actions_in=np.ascontiguousarray(acts.transpose(0, 2, 1)), **kw)
    else:
        judge, _ = S._oracle(name, policy)
        rec, _, _ = O.rollout(N, STEPS, action_seed=c["action_seed"], policy=S.POLICY[policy], **kw)
    # the dynamics do not depend on the weights; configurations A and F flag nothing
    assert P.bits_equal(rec["results"], judge["results"]) and P.bits_equal(rec["obs_i32"], judge["obs_i32"])
    assert not (rec["status"] & FLAGS).any()
    if sname is None:
        assert P.bits_equal(rec["rewards"], judge["rewards"])
    r = np.ascontiguousarray(rec["rewards"])
    r.setflags(write=False)
    return r


def _expected(name, policy, segments=SEGMENTS):
    want = np.empty((STEPS, N, 8))
    for t0, t1, sname in segments:
        want[t0:t1] = _oracle_w(name, policy, sname)[t0:t1]
    return want


def _floor(name, policy, rec, what):
    """The per-term counts of the oracle's records, printed, and the floor on them."""
    cnt = P.reward_term_counts(rec, (np.asarray(rec["status"]) & FLAGS) == 0)
    print(f"rewards {what} cfg {name} {policy}: env-steps per term {cnt}")
    if name == "F":
        P.reward_conditions(cnt, P.REWARD_UNREACHABLE_F[policy], what, exempt=P.REWARD_EXEMPT_F)
    else:
        P.reward_conditions(cnt, P.REWARD_UNREACHABLE[policy], what)
    return cnt


def _assert_rewards(got, want, what, segments=SEGMENTS):
    """got, want f64 [T, N, 8]: byte-equal, with the first differing (step, env, agent) otherwise."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint64) != want.view(np.uint64)
    if bad.any():
        t, e, a = (int(x) for x in np.argwhere(bad)[0])
        sname = [s for t0, t1, s in segments if t0 <= t < t1]
        raise AssertionError((what, "rewards differ first at (step, env, agent)", (t, e, P.AGENT_NAMES[a]), sname,
                              float(got[t, e, a]), float(want[t, e, a]), int(bad.sum()), "of", bad.size,
                              "per agent", bad.sum((0, 1)).tolist()))


def _np(b, keys):
    """The first N envs of a Buffers' outputs as numpy, env-major rows [T, N, F] / [T, N]."""
    out = {}
    for k in keys:
        v = getattr(b, k)[..., :N]
        out[k] = (v.transpose(1, 2) if v.dim() == 3 else v).contiguous().cpu().numpy()
    return out


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _set(env, sname):
    if sname is not None:
        got = env.set_reward_weights(P.REWARD_SETS[sname])
        assert tuple(got.values()) == tuple(P.REWARD_SETS[sname]) == tuple(env.reward_weights().values())


def _fused_run(G, name, policy, kernel, n, infos, opts, weighted):
    """One fused-launch path: the launches (a weight set before each when `weighted`), snapshot ->
    restore into a fresh handle (TAIL_SET set there) -> TAIL more steps; the lean outputs and the
    status words of the first N envs."""
    c = P.STATUS_CFGS[name]
    keys = S.LEAN + ("status",)
    env = S._env(G, name, n, **opts)
    parts, t = [], 0
    for k, sname in zip(CHUNKS, SETS):
        _set(env, sname if weighted else None)
        b = env.rollout(k, action_seed=c["action_seed"], step0=t, policy=policy, infos=infos)
        parts.append(_np(b, keys))
        t += k
    assert env.last_kernel() == kernel, env.last_kernel()
    snap = env.snapshot()
    env2 = S._env(G, name, n, **opts)
    env2.restore(snap)
    _set(env2, TAIL_SET if weighted else None)
    b = env2.rollout(TAIL, action_seed=c["action_seed"], step0=t, policy=policy, infos=infos)
    parts.append(_np(b, keys))
    assert env2.last_kernel() == kernel, env2.last_kernel()
    assert env.faults() == 0 and env2.faults() == 0
    return _cat(parts)


def _check(name, policy, got, base, what):
    """got: the weighted run, base: the same path under the default weights."""
    assert not (got["status"] & 1).any() and not (base["status"] & 1).any(), what      # A, F flag none
    _assert_rewards(base["rewards"], _oracle_w(name, policy, None), what + " (default weights)")
    _assert_rewards(got["rewards"], _expected(name, policy), what)
    for k in OTHERS:
        assert P.bits_equal(got[k], base[k]), (what, k, "changed with the weights")
    assert (got["rewards"] != base["rewards"]).mean() > 0.9          # the sets are not the defaults


def _fused_path(G, policy, kernel, what, n=N, infos=False, name="A", **opts):
    judge, _ = S._oracle(name, policy)
    _floor(name, policy, judge, what)
    got = _fused_run(G, name, policy, kernel, n, infos, opts, True)
    base = _fused_run(G, name, policy, kernel, n, infos, opts, False)
    _check(name, policy, got, base, what)


@pytest.mark.parametrize("epw", [16, 32, 64])
def test_rewards_agents(G, epw):
    """k_step_ag<lds,predraw> (uniform-random actions) at 16 / 32 / 64 envs per workgroup: ag_emit's
    table index from the halves AM and the packaging wave wrote."""
    _fused_path(G, "random", S.AG, f"k_step_ag<{epw}>", agents=1, ag_envs=epw)


@pytest.mark.parametrize("policy", ["random", "masked"])
@pytest.mark.parametrize("variant", list(S.PIPES))
def test_rewards_pipe(G, variant, policy):
    """k_step_pipe's five variants (the one-emit-wave ones at 16 448 envs, compared on their first
    200): the emit wave's flags and action from the packed snapshot word."""
    n, opts = S.PIPES[variant]
    _fused_path(G, policy, f"k_step_pipe<{variant}>", f"k_step_pipe<{variant}>", n=n, **opts)


def test_rewards_pipe_blue2(G):
    """k_step_pipe<lds,2emit,predraw> under masked actions on configuration F, where
    packaging_blue_2 earns each of its three terms (31 / 161 / 68 env-steps in the oracle)."""
    n, opts = S.PIPES["lds,2emit,predraw"]
    _fused_path(G, "masked", "k_step_pipe<lds,2emit,predraw>", "k_step_pipe<lds,2emit,predraw>", n=n, name="F", **opts)


MANY = [("k_step_many<lds,full>", True, {}), ("k_step_many<full>", True, dict(fused_lds=0)),
        ("k_step_many<lds>", False, dict(pipeline=0))]


@pytest.mark.parametrize("policy", ["random", "masked"])
@pytest.mark.parametrize("kernel,infos,opts", MANY)
def test_rewards_many(G, kernel, infos, opts, policy):
    """The single-wave k_step_many (env_advance's rewards): LDS and global tables, full and lean."""
    _fused_path(G, policy, kernel, kernel, infos=infos, **opts)


@pytest.mark.parametrize("kernel", ["k_step_many<lds>", "k_step_pipe<lds,2emit,predraw>"])
def test_rewards_heuristic(G, kernel):
    """The heuristic policy, the only one that completes orders by the hundred (ORDER_COMPLETE and
    THROUGHPUT on > 500 env-steps), on one k_step_many and one k_step_pipe variant."""
    opts = dict(pipeline=0) if "many" in kernel else S.PIPES["lds,2emit,predraw"][1]
    _fused_path(G, "heuristic", kernel, kernel, **opts)


def _host_run(G, env, acts, t0, server, weighted, segments):
    """fjsp_step, or the step server, over rows [t0, t0 + len(acts)) of the host action stream,
    like test_gpu_status._host_steps; a segment's weight set is set right before its first step --
    on the server while it is running, which quiesces it (the next server_step relaunches)."""
    keys = S.LEAN + ("status",)
    n = env.num_envs
    out = {k: [] for k in keys}
    if server:
        hb = torch.zeros(8, n, dtype=torch.uint8).pin_memory()
        b = env.server_start(hb, autoreset=True, buffers=G.vec_env.Buffers(1, n, env.device, infos=True, next_obs=True))
        assert env.last_kernel() == "k_step_server"
    else:
        b = G.vec_env.Buffers(1, n, env.device, infos=True, next_obs=True)
        acts_d = torch.from_numpy(np.array(acts)).to(env.device)
    starts = {s0: sname for s0, _, sname in segments}
    for i in range(len(acts)):
        if weighted and t0 + i in starts:
            _set(env, starts[t0 + i])
        if server:
            hb.numpy()[:] = acts[i]
            env.server_step()
            torch.cuda.current_stream().synchronize()
        else:
            env.step(acts_d[i], buffers=b)
        for k, v in _np(b, keys).items():
            out[k].append(v)
    if server:
        assert env.last_kernel() == "k_step_server"
        env.server_stop()
    else:
        assert env.last_kernel() == "k_step<canon>"
    return {k: np.concatenate(v) for k, v in out.items()}


@pytest.mark.parametrize("path", ["step64", "step16", "server"])
@pytest.mark.parametrize("name", ["A", "F"])
def test_rewards_host_actions(G, name, path):
    """fjsp_step (64 and 16 envs per workgroup) and the step server with the oracle's masked-random
    action stream, judged by the oracle's weighted replays of that stream.  The weights change
    between two steps (on the running server: it quiesces and relaunches), then snapshot, restore
    into a fresh handle with DISTINCT, the last TAIL steps.  Configuration F: the one in which
    packaging_blue_2 earns its terms."""
    acts, judge = S._oracle_actions(name)
    _floor(name, "masked", judge, path)
    server = path == "server"
    opts = {} if server else dict(step_envs=int(path[4:]))
    T0 = sum(CHUNKS)
    runs = []
    for weighted in (True, False):
        env = S._env(G, name, **opts)
        a = _host_run(G, env, acts[:T0], 0, server, weighted, SEGMENTS)
        snap = env.snapshot()
        env2 = S._env(G, name, **opts)
        env2.restore(snap)
        b = _host_run(G, env2, acts[T0:], T0, server, weighted, SEGMENTS)
        assert env.faults() == 0 and env2.faults() == 0
        runs.append(_cat([a, b]))
    _check(name, "host", runs[0], runs[1], path)


# The learner's seed of test_rewards_a2c_collect.  An untrained network's policy is far from uniform
# and differs from seed to seed: over seeds 5..24 the smallest count of a masked-reachable term in
# the oracle's replay of the 280 sampled steps is 0 (four seeds) to 60; seed 5, which the status
# test uses on configuration A, completes orders on 6 env-steps only.  15: orders_completed 50,
# pkg_green.complete 54, every other reachable term >= 91; nothing flagged.
COLLECT_SEED = 15


def test_rewards_a2c_collect(G):
    """The A2C collect (k_policy_step, captured graphs on, two env groups): four batches of 70
    steps; DISTINCT is set before the first (eager) and holds for the second (captured, replayed),
    SCALED is set before the third and fourth, which replay the graph captured under DISTINCT: the
    replayed launches read the device table, not a captured copy.  Judged by the oracle's weighted
    replays of the sampled actions."""
    A = importlib.import_module("multi-agent-rl-for-fjsp_amd.a2c_vec")
    c = P.STATUS_CFGS["A"]
    T, sets = 70, ("DISTINCT", "DISTINCT", "SCALED", "SCALED")
    env = G.make_env(N, **c["cfg"])
    L = A.VecMultiAgentA2C(env, batch_size=T, seed=COLLECT_SEED, use_graph=True)
    L.reset(seeds=torch.from_numpy(P.status_seeds(N).astype(np.int64)), num_orders=c["num_orders"])
    acts, rew, st = [], [], []
    for i, sname in enumerate(sets):
        if i == 0 or sname != sets[i - 1]:
            torch.cuda.synchronize()
            _set(env, sname)
        L.collect()
        torch.cuda.synchronize()
        assert env.last_kernel() == "k_policy_step" and (L._graph is not None) == (i >= 1)
        b = L._bufs
        acts.append(b["actions"][:T].cpu().numpy())
        rew.append(b["rewards"][:T].cpu().numpy().transpose(0, 2, 1))
        st.append(b["status"][:T].cpu().numpy().view(np.uint32))
        L.roll_over()
    acts, rew, st = np.concatenate(acts), np.concatenate(rew), np.concatenate(st)
    assert env.faults() == 0 and not (st & 1).any()
    ain = np.ascontiguousarray(acts.transpose(0, 2, 1))
    kw = dict(seeds=P.status_seeds(N), num_orders=c["num_orders"], actions_in=ain, **c["cfg"])
    judge, _, _ = O.rollout(N, 4 * T, **kw)
    assert not (judge["status"] & FLAGS).any()
    _floor("A", "masked", judge, "k_policy_step (learner seed %d)" % COLLECT_SEED)
    want = np.empty_like(rew)
    segs = []
    for i, sname in enumerate(sets):
        if i == 0 or sname != sets[i - 1]:
            rec, _, _ = O.rollout(N, 4 * T, weights=P.REWARD_SETS[sname], **kw)
        want[i * T:(i + 1) * T] = rec["rewards"][i * T:(i + 1) * T]
        segs.append((i * T, (i + 1) * T, sname))
    _assert_rewards(np.ascontiguousarray(rew), want, "k_policy_step", segs)
    assert (rew != judge["rewards"]).mean() > 0.9


def test_restored_fresh_handle_has_default_weights(G):
    """The weights belong to the handle and are not part of a snapshot: a snapshot of a handle
    running under DISTINCT, restored into a fresh handle on which set_reward_weights is never
    called, continues with default-weight rewards (include/fjsp.h)."""
    c = P.STATUS_CFGS["A"]
    K = CHUNKS[0]
    env = S._env(G, "A", agents=1)
    _set(env, "DISTINCT")
    a = _np(env.rollout(K, action_seed=c["action_seed"], step0=0, policy="random"), ("rewards",))["rewards"]
    _assert_rewards(a, _oracle_w("A", "random", "DISTINCT")[:K], "before the snapshot")
    env2 = S._env(G, "A", agents=1)
    env2.restore(env.snapshot())
    assert tuple(env2.reward_weights().values()) == P.DEFAULT_WEIGHTS
    b = _np(env2.rollout(TAIL, action_seed=c["action_seed"], step0=K, policy="random"), ("rewards",))["rewards"]
    assert env2.last_kernel() == S.AG and env.faults() == 0 and env2.faults() == 0
    _assert_rewards(b, _oracle_w("A", "random", None)[K:K + TAIL], "restored fresh handle")
    assert (b != _oracle_w("A", "random", "DISTINCT")[K:K + TAIL]).mean() > 0.9


def test_set_reward_weights_surface(G):
    """FJSPVecEnv.set_reward_weights / reward_weights: single fields by name (either case), a
    mapping, a fjsp_reward_weights and sixteen values give the same table as the C call through
    ctypes; unknown names and wrong lengths are refused and change nothing."""
    import ctypes
    c = P.STATUS_CFGS["A"]
    nat = G.native
    K = 30

    def run(setter):
        env = S._env(G, "A", 64)
        setter(env)
        r = _np64(env.rollout(K, action_seed=c["action_seed"], step0=0, policy="masked"))
        return env, r

    def _np64(b):
        return b.rewards.transpose(1, 2).contiguous().cpu().numpy()

    d = dict(zip(nat.REWARD_FIELDS, P.DISTINCT))
    want = _oracle_w("A", "masked", "DISTINCT")[:K, :64]
    env, r = run(lambda e: e.set_reward_weights(**{k.upper(): v for k, v in d.items()}))
    assert env.reward_weights() == d
    _assert_rewards(r, want, "names")
    for setter in (lambda e: e.set_reward_weights(d), lambda e: e.set_reward_weights(nat.fjsp_reward_weights(*P.DISTINCT)),
                   lambda e: e.set_reward_weights(list(P.DISTINCT)),
                   lambda e: nat.check(nat.lib().fjsp_set_reward_weights(
                       e.handle, ctypes.byref(nat.fjsp_reward_weights(*P.DISTINCT))))):
        _assert_rewards(run(setter)[1], want, "setter")
    env = S._env(G, "A", 64)
    assert tuple(env.reward_weights().values()) == P.DEFAULT_WEIGHTS
    one = env.set_reward_weights(agv_move_penalty=-0.77)
    assert one["agv_move_penalty"] == -0.77 and sum(a != b for a, b in zip(one.values(), P.DEFAULT_WEIGHTS)) == 1
    with pytest.raises(ValueError):
        env.set_reward_weights(agv_move_penalti=1.0)
    with pytest.raises(ValueError):
        env.set_reward_weights([1.0] * 15)
    assert env.reward_weights() == one
