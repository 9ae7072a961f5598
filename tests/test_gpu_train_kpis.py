"""KPIs of the training rollouts (track_kpis=True): the fused collect's KPI instance
(k_policy_step<STAGED, KPI>: result words, the stations' int8 observations, infos, sim time)
against the two-launch collect byte for byte and against the oracle, the learner's KPI log against
kpi_reference and the episode log, learn()'s training_kpis, and fjsp_a2c_policy_step's argument
checks.  Sizes as tests/test_gpu_episodes.py::_learner_run: 30-step episodes of 3 orders, 5
batches of 16 vector steps, env seeds arange(n) + 9, so every env ends at least two episodes by
truncation alone."""
import ctypes
import functools
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from oracle import oracle as O  # noqa: E402
from tests import kpi_util as KU  # noqa: E402
from tests import parity_util as P  # noqa: E402

K = KU.kpis
T, ROUNDS, NUM_ORDERS, MAX_STEPS = 16, 5, 3, 30
BASE_KEYS = ("feats", "masks", "actions", "values", "rewards", "term", "trunc", "status")
KPI_KEYS = ("results", "obs_i8", "orders_completed", "packaged", "sim_time")
MESSAGE = ("fjsp_a2c_policy_step: outputs limited to rewards, term, trunc, status, next_masks, feats, "
           "results, obs_i8, orders_completed, packaged, sim_time")


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util  # noqa: F401
    return {"A": importlib.import_module("multi-agent-rl-for-fjsp_amd.a2c_vec"),
            "P": importlib.import_module("multi-agent-rl-for-fjsp_amd.ppo_vec"),
            "V": importlib.import_module("multi-agent-rl-for-fjsp_amd.vec_env"),
            "nat": importlib.import_module("multi-agent-rl-for-fjsp_amd._native")}


def _learner(M, n, kpis, fused=True, groups=2, graph=None, episodes=False, ppo=False, max_steps=MAX_STEPS):
    env = M["V"].FJSPVecEnv(n, max_episode_steps=max_steps)
    kw = dict(batch_size=T, seed=1, use_graph=graph, track_episodes=episodes)
    if kpis is not None:   # None: the constructor as it was before the switch existed
        kw["track_kpis"] = kpis
    L = M["P"].VecMultiAgentPPO(env, ppo_epochs=2, **kw) if ppo else M["A"].VecMultiAgentA2C(env, **kw)
    L.fused_step = fused
    L.collect_groups = groups
    return L


@functools.lru_cache(maxsize=None)
def _run_cached(n, kpis, fused, groups, graph, episodes, ppo, orders, max_steps, base):
    M_ = _run_cached.M
    L = _learner(M_, n, kpis, fused, groups, graph, episodes, ppo, max_steps)
    L.reset(seeds=torch.arange(n) + base, num_orders=orders)
    slabs = []
    for _ in range(ROUNDS):
        L.collect()
        if episodes:
            L.account_episodes()
        if kpis:
            L.account_kpis()
        slabs.append({k: L._bufs[k].clone() for k in BASE_KEYS + KPI_KEYS if k in L._bufs})
        L.update()
        L.roll_over()
    params = [p.detach().clone() for p in list(L.actors.parameters()) + list(L.critic.parameters())]
    return L, slabs, params, L.env.last_kernel()


def _run(M, n, kpis=True, fused=True, groups=2, graph=False, episodes=False, ppo=False, orders=NUM_ORDERS,
         max_steps=MAX_STEPS, base=9, own=False):
    """One learner over the 5 batches (computed once per configuration, shared, left unchanged; own:
    a run of the caller's own, whose logs it may drain): the learner, a copy of every slab after
    every collect, the final parameters, the env's last kernel."""
    _run_cached.M = M
    f = _run_cached.__wrapped__ if own else _run_cached
    return f(n, kpis, fused, groups, graph, episodes, ppo, orders, max_steps, base)


def _cat(slabs, k):
    return torch.cat([s[k] for s in slabs]).cpu().numpy()


# ------------------------------------------------------------------ 1. fused == two launches
@pytest.mark.parametrize("n,groups,graph", [(64, 1, False), (128, 2, False), (130, 2, False), (128, 1, True)])
def test_fused_collect_equals_two_launches_on_the_kpi_slabs(M, n, groups, graph):
    """track_kpis=True, the fused collect against policy kernel + fjsp_step: every byte of every
    slab, the five KPI slabs included, over all 5 batches.  One full tile (staged instance), two
    streams, a partial tile (130: every tile takes the unstaged instance), and an eager batch, the
    capture and three replays."""
    _, two, _, k2 = _run(M, n, fused=False, groups=groups, graph=graph)
    _, one, _, k1 = _run(M, n, fused=True, groups=groups, graph=graph)
    assert k1 == "k_policy_step" and k2.startswith("k_step")
    for b in range(ROUNDS):
        assert set(one[b]) == set(two[b]) == set(BASE_KEYS + KPI_KEYS)
        for k in BASE_KEYS + KPI_KEYS:
            assert torch.equal(one[b][k], two[b][k]), (b, k)
    ends = _cat(one, "term") | _cat(one, "trunc")
    assert ends.sum(0).min() >= 2                        # every env crossed two auto-resets
    assert _cat(one, "results").any() and _cat(one, "obs_i8").any() and (_cat(one, "sim_time") > 0).all()


# ------------------------------------------------------------------ 2. against the oracle
def _oracle_replay(slabs, envs, base=9, orders=NUM_ORDERS, max_steps=MAX_STEPS):
    """The slabs' recorded actions of `envs` through the oracle from the seeds they were reset with,
    across their auto-resets: the five KPI outputs and the flags at every step; returns the
    episode ends met."""
    acts = _cat(slabs, "actions")
    got = {k: _cat(slabs, k) for k in KPI_KEYS + ("term", "trunc")}
    res = got["results"].view(np.uint32)
    ends = 0
    for e in envs:
        o = O.OracleEnv(max_episode_steps=max_steps)
        o.reset(seed=base + e, num_orders=orders)
        for t in range(ROUNDS * T):
            r = o.step(acts[t, :, e])
            assert P.bits_equal(res[t, :, e], r["results"]), (e, t, "results")
            assert P.bits_equal(got["obs_i8"][t, :, e], r["obs_i8"]), (e, t, "obs_i8")
            assert int(got["orders_completed"][t, e]) == int(r["orders_completed"]), (e, t)
            assert int(got["packaged"][t, e]) == int(r["packaged"]), (e, t)
            assert P.bits_equal(got["sim_time"][t, e], r["sim_time"]), (e, t, "sim_time")
            assert (int(got["term"][t, e]), int(got["trunc"][t, e])) == (int(r["term"]), int(r["trunc"])), (e, t)
            if r["term"] or r["trunc"]:
                ends += 1
                o.reset(num_orders=orders)
    return ends


@pytest.mark.parametrize("n,envs", [(130, (0, 63, 64, 127, 128, 129)), (64, (0, 31, 63))])
def test_kpi_slabs_equal_the_oracle(M, n, envs):
    """The recorded actions of the fused collect replayed through the oracle, with the seeds the
    envs were reset with, across their auto-resets: result words, the twelve int8 fields of the
    post-step state, both infos and sim_time at every step.  n = 130: the unstaged instance, envs
    128 and 129 in the partial tile; n = 64: the staged instance."""
    _, slabs, _, _ = _run(M, n, fused=True, groups=2 if n == 130 else 1)
    assert _oracle_replay(slabs, envs) >= 2 * len(envs)


# ------------------------------------------------------------------ 3. tracking does not perturb training
@pytest.mark.parametrize("ppo", [False, True])
def test_kpi_tracking_does_not_perturb_training(M, ppo):
    """Slabs and final parameters with track_kpis=True equal those of a learner built without the
    switch, bit for bit (A2C, and PPO with ppo_epochs=2)."""
    _, s1, p1, _ = _run(M, 128, kpis=True, ppo=ppo)
    L0, s0, p0, _ = _run(M, 128, kpis=None, ppo=ppo)
    assert L0.kpi_log is None and not any(k in L0._bufs for k in KPI_KEYS)
    for b in range(ROUNDS):
        assert set(s0[b]) == set(BASE_KEYS)
        for k in BASE_KEYS:
            assert torch.equal(s1[b][k], s0[b][k]), (b, k)
    assert len(p1) == len(p0)
    for a, b in zip(p1, p0):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ 4. records
# (num_orders, max_episode_steps, first env seed).  The first case has the sizes of every other test
# here; no episode of it can terminate (see the test's docstring), so the second one exists for the
# terminated records: its env seeds were picked on the two-launch collect, as it was before the KPI
# instance existed, among arange(128) + {9, 1009, ..., 9009}.
RECORD_CASES = {"truncated": (NUM_ORDERS, MAX_STEPS, 9), "terminated": (1, 60, 2009)}


@pytest.mark.parametrize("case", list(RECORD_CASES))
def test_training_records_equal_reference_and_join_the_episode_log(M, case):
    """pop_kpis() after the 5 batches == kpi_reference over the concatenated slabs, byte for byte;
    the 40-byte heads == the episode log's records index by index, which now carry real
    orders_completed / packaged on the fused path.  n = 128, learner seed 1.

    Observed on the two-launch collect before this feature (and again with it, on both collects):
    "truncated" (3 orders, 30-step episodes, env seeds arange(128) + 9) 256 records, 256 truncated,
    0 terminated; "terminated" (1 order, 60-step episodes, env seeds arange(128) + 2009) 128
    records, 126 truncated, 2 terminated.  Three orders cannot be completed in 30 steps: over 8 192
    such episodes the oracle's heuristic policy completes at most two of them, and uniform masked
    actions completed one order in 2 of 65 536 episodes and never three; so at those sizes only the
    truncated records can be asserted to exist (for every env), and the terminated ones are
    asserted in the second case, which is also the one whose episodes reach the packaging
    stations' int8 fields."""
    n = 128
    orders, max_steps, base = RECORD_CASES[case]
    L, slabs, _, kern = _run(M, n, kpis=True, episodes=True, orders=orders, max_steps=max_steps, base=base, own=True)
    assert kern == "k_policy_step"
    slab = {k: _cat(slabs, k) for k in KU.KEYS}
    slab["results"] = slab["results"].view(np.uint32)
    want, carry = KU.reference(slab)
    er, edrop = L.episode_log.pop_records()
    kp = L.pop_kpis()
    assert kp["dropped"] == 0 and edrop == 0
    KU.same(kp["records"], want)
    assert L.kpi_log.carry.cpu().numpy().tobytes() == carry.tobytes()
    assert L.kpi_log.step0 == ROUNDS * T
    assert len(er) == len(want) and KU.heads(er).tobytes() == KU.heads(kp["records"]).tobytes()
    assert (er["orders_completed"] >= 0).all() and (er["packaged"] >= 0).all()
    trunc, term = kp["truncated"], kp["terminated"]
    print(case, "records", len(want), "truncated", int(trunc.sum()), "terminated", int(term.sum()))
    assert trunc.sum() > 0
    if case == "truncated":
        assert np.bincount(kp["env"][trunc], minlength=n).min() >= 2      # truncated records for every env
    else:
        assert term.sum() > 0
        assert (kp["orders_completed"][term] == orders).all() and (kp["packaged"][term] > 0).all()
        # the episodes that terminate went through the packaging stations: their int8 fields are
        # not all zero here, the two-launch collect wrote the same bytes, and so did the oracle
        assert slab["obs_i8"][:, 4:].any()
        _, two, _, _ = _run(M, n, kpis=True, fused=False, orders=orders, max_steps=max_steps, base=base)
        for b in range(ROUNDS):
            for k in BASE_KEYS + KPI_KEYS:
                assert torch.equal(slabs[b][k], two[b][k]), (b, k)
        envs = sorted(set(kp["env"][term].tolist()))
        assert _oracle_replay(slabs, envs, base, orders, max_steps) >= len(envs)
    assert (kp["makespan"] == kp["length"] * 10.0).all()
    assert L.training_kpis["records"].tobytes() == want.tobytes()
    assert len(L.pop_kpis()["records"]) == 0                          # drained
    assert L.training_kpis["records"].tobytes() == want.tobytes()
    assert L.training_kpis["agents"].shape == (8, 8, len(want))


# ------------------------------------------------------------------ 5. learn()
def test_learn_fills_training_kpis(M):
    """learn() over 5 batches with both logs: training_kpis holds one record per entry of
    overall_rewards, in the same order (the episode log's end steps, and the records of the same
    batches scanned by hand); the curve comes out of kpi_summary; PPO's epochs do not scan a
    batch again; a learner without the switch has no log."""
    n = 128
    L = _learner(M, n, True, episodes=True)
    assert L.learn(ROUNDS * T * n, num_orders=NUM_ORDERS, seeds=torch.arange(n) + 9) is L
    tk = L.training_kpis
    assert len(tk["records"]) == len(L.overall_rewards) >= 2 * n
    assert (tk["end_step"] * n).tolist() == L.episode_end_timesteps
    assert tk["dropped"] == 0 and L.kpi_log.step0 == ROUNDS * T
    _, slabs, _, _ = _run(M, n, kpis=True, episodes=True)
    slab = {k: _cat(slabs, k) for k in KU.KEYS}
    slab["results"] = slab["results"].view(np.uint32)
    want, _ = KU.reference(slab)
    assert tk["records"].tobytes() == want.tobytes()
    curve = K.kpi_summary(tk["records"])
    assert curve["makespan"].shape == (len(want),) and (curve["utilisation"] <= 1.0).all()
    # PPO: one scan per collected batch whatever the epochs
    Lp = _learner(M, n, True, episodes=True, ppo=True)
    Lp.learn(ROUNDS * T * n, num_orders=NUM_ORDERS, seeds=torch.arange(n) + 9)
    assert Lp.kpi_log.step0 == ROUNDS * T
    assert len(Lp.training_kpis["records"]) == len(Lp.overall_rewards) >= 2 * n
    # ... and the first batch (the same actions under both learners) yields the same records
    first = []
    for ppo in (False, True):
        L1 = _learner(M, n, True, ppo=ppo)
        L1.learn(T * n, num_orders=NUM_ORDERS, seeds=torch.arange(n) + 9)
        assert L1.kpi_log.step0 == T
        first.append(L1.training_kpis["records"])
    assert first[0].tobytes() == first[1].tobytes()
    off = _learner(M, n, None)
    assert off.kpi_log is None and off.track_kpis is False and off.training_kpis is None


# ------------------------------------------------------------------ 6. argument checks
def test_policy_step_argument_checks(M):
    """fjsp_a2c_policy_step still rejects obs_i32 / obs_f32 / masks / next_* with an error that
    names the accepted set, and runs with `results` as its only output."""
    nat = M["nat"]
    n = 64
    L = _learner(M, n, False, groups=1)
    L.reset(seeds=torch.arange(n) + 9, num_orders=NUM_ORDERS)
    b = L._bufs
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.env._sync_stream()

    def call(o):
        return nat.lib().fjsp_a2c_policy_step(L.env.handle, ptr(b["feats"][0]), ptr(b["masks"][0]), ptr(L._pw_actor),
                                              ptr(L._pw_critic), ptr(L._rng), 0, 0, 0, ptr(b["actions"][0]),
                                              ptr(b["values"][0]), 1, ctypes.byref(o), 0, n, stream)
    spare = torch.zeros(38 * n, dtype=torch.int32, device="cuda")
    for field in ("obs_i32", "next_i8", "obs_f32", "masks", "next_i32", "next_f32"):
        o = nat.fjsp_out()
        o.results = spare.data_ptr()
        setattr(o, field, spare.data_ptr())
        assert call(o) != 0, field
        assert nat.lib().fjsp_last_error().decode() == MESSAGE, field
    torch.cuda.synchronize()
    assert not spare.any() and not b["actions"][0].any()            # nothing was launched
    res = torch.zeros(8, n, dtype=torch.int32, device="cuda")
    o = nat.fjsp_out()
    o.results = res.data_ptr()
    assert call(o) == 0, nat.lib().fjsp_last_error()
    torch.cuda.synchronize()
    assert L.env.last_kernel() == "k_policy_step"
    assert res.any()                                                # result words were written
