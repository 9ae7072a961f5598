"""Episode accounting on the GPU (fjsp_episode_scan, episodes.EpisodeLog) against
episodes_reference, the host restatement of a2c.py:311-313 / :348, byte for byte on every field:
the reference's recorded traces through the kernel, synthetic edge slabs, the capacity bound,
appending without synchronisation, FJSPVecEnv.evaluate_episodes and the tracking learner."""
import ctypes
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from tests import episodes_util as U  # noqa: E402

E = U.episodes


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util  # noqa: F401
    return {"A": importlib.import_module("multi-agent-rl-for-fjsp_amd.a2c_vec"),
            "V": importlib.import_module("multi-agent-rl-for-fjsp_amd.vec_env"),
            "nat": importlib.import_module("multi-agent-rl-for-fjsp_amd._native")}


def _dev(slab, infos=True):
    d = {k: torch.from_numpy(v).cuda() for k, v in slab.items()}
    return (d["rewards"], d["term"], d["trunc"]) + ((d["orders_completed"], d["packaged"]) if infos else ())


def _scan_split(log, slab, rows, infos=True):
    T = slab["rewards"].shape[0]
    for lo, hi in U.cuts(T, rows):
        log.scan(*_dev(U.rows_of(slab, lo, hi), infos))


def _same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in E.REC_DTYPE.names:
        assert got[f].tobytes() == want[f].tobytes(), f
    assert got.tobytes() == want.tobytes()


def _carry(log):
    return log.acc.cpu().numpy(), log.len.cpu().numpy()


# ------------------------------------------------------------------ 1. golden replay
@pytest.mark.parametrize("infos", [True, False])
@pytest.mark.parametrize("rows", (1000,) + U.SPLITS)
def test_golden_traces_through_the_kernel(M, rows, infos):
    slab = U.trace_slab()
    want, acc, ln = U.trace_reference(infos)
    assert len(want) == 71
    log = E.EpisodeLog(12, "cuda", capacity=128)
    _scan_split(log, slab, rows, infos)
    got, dropped = log.pop_records()
    assert dropped == 0
    _same(got, want)
    a, n_open = _carry(log)
    assert a.tobytes() == acc.tobytes() and n_open.tolist() == ln.tolist()
    assert log.step0 == 1000


# ------------------------------------------------------------------ 2. ordering and edges
@pytest.mark.parametrize("N", [130, 1, 64])
def test_synthetic_ordering_and_edges(M, N):
    slab = U.synthetic_slab(N)
    want, acc, ln = U.reference(slab, env_gid0=1000, step0=0)
    done = (slab["term"] | slab["trunc"]).astype(bool)
    assert not done[5].any() and done[11].all() and done[0].any() and done[-1].any()
    log = E.EpisodeLog(N, "cuda", capacity=len(want) + 3, env_id_base=1000)
    log.scan(*_dev(slab))
    got, dropped = log.pop_records()
    assert dropped == 0
    _same(got, want)
    a, n_open = _carry(log)
    assert a.tobytes() == acc.tobytes() and n_open.tolist() == ln.tolist()
    # a second slab continues the open episodes from the carry
    want2, _, _ = U.reference(slab, acc=acc, length=ln, step0=37, env_gid0=1000, seq0=len(want))
    log.scan(*_dev(slab))
    _same(log.pop_records()[0], want2)


# ------------------------------------------------------------------ 3. capacity
def test_capacity_bounds_the_writes(M):
    nat = M["nat"]
    N, cap, guard = 130, 5, 64
    slab = U.synthetic_slab(N)
    want, _, _ = U.reference(slab)
    assert len(want) > cap + guard
    T = slab["rewards"].shape[0]
    size = E.REC_DTYPE.itemsize
    buf = torch.full(((cap + guard) * size,), 0xA5, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(8, N, dtype=torch.float64, device="cuda")
    ln = torch.zeros(N, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    temp = torch.empty(E.temp_bytes(T, N), dtype=torch.uint8, device="cuda")
    r, te, tr, oc, pk = _dev(slab)
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    nat.check(nat.lib().fjsp_episode_scan(P(r), P(te), P(tr), P(oc), P(pk), T, N, 0, 0, P(acc), P(ln), P(buf), cap,
                                          P(count), P(temp), temp.numel(),
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    raw = buf.cpu().numpy()
    assert int(count.item()) == len(want)
    _same(raw[:cap * size].view(E.REC_DTYPE), want[:cap])
    assert (raw[cap * size:] == 0xA5).all()
    # the same through the log: pop() reports what did not fit
    log = E.EpisodeLog(N, "cuda", capacity=cap)
    log.scan(r, te, tr, oc, pk)
    got = log.pop()
    assert got["dropped"] == len(want) - cap and len(got["total"]) == cap
    assert got["total"].tobytes() == want["total"][:cap].tobytes()
    # the log is empty again and keeps appending from its start
    log.scan(r, te, tr, oc, pk)
    again = log.pop()
    assert again["seq"].tolist() == list(range(len(want), len(want) + cap))


# ------------------------------------------------------------------ 4. append without sync
def test_two_scans_append_without_synchronising(M):
    N = 130
    a, b = U.synthetic_slab(N), U.synthetic_slab(N, seed=77)
    both = {k: np.concatenate([a[k], b[k]]) for k in a}
    want, _, _ = U.reference(both)
    log = E.EpisodeLog(N, "cuda", capacity=len(want))
    log.scan(*_dev(a))
    log.scan(*_dev(b))
    got, dropped = log.pop_records()
    assert dropped == 0
    assert got["seq"].tolist() == list(range(len(want)))
    _same(got, want)            # end_step = step0 + t + 1 with step0 = 37 for the second slab


# ------------------------------------------------------------------ 5. on the env
def test_evaluate_episodes_on_the_env(M):
    V = M["V"]
    n, steps, chunk = 128, 450, 64
    seeds = torch.arange(n) * 5 + 2
    got = V.FJSPVecEnv(n).evaluate_episodes("heuristic", num_orders=2, steps=steps, seeds=seeds, chunk=chunk)
    # a second, identical run through rollout, its slabs kept
    env = V.FJSPVecEnv(n)
    env.reset(seeds=seeds, num_orders=2)
    keep = []
    for lo, hi in U.cuts(steps, chunk):
        b = env.rollout(hi - lo, step0=lo, policy="heuristic", autoreset=True, infos=True)
        keep.append({k: getattr(b, k).cpu().numpy() for k in ("rewards", "term", "trunc", "orders_completed",
                                                              "packaged")})
    slab = {k: np.concatenate([s[k] for s in keep]) for k in keep[0]}
    want, _, _ = U.reference(slab)
    assert got["dropped"] == 0 and len(want) >= 2 * n
    wd = E.records_dict(want)
    for k in wd:
        assert np.asarray(got[k]).tobytes() == np.asarray(wd[k]).tobytes(), k
    assert (got["orders_completed"][got["terminated"]] == 2).all()


def test_first_episode_equals_evaluate(M):
    V = M["V"]
    n, steps = 128, 450
    seeds = torch.arange(n) * 5 + 2
    ev = V.FJSPVecEnv(n).evaluate("heuristic", num_orders=2, max_steps=steps, seeds=seeds)
    env = V.FJSPVecEnv(n)
    env.reset(seeds=seeds, num_orders=2)
    b = env.rollout(steps, policy="heuristic", autoreset=False, infos=True)
    log = E.EpisodeLog(n, env.device, capacity=n * steps)
    log.scan(b.rewards, b.term, b.trunc, b.orders_completed, b.packaged)
    rec = log.pop()
    ended = (b.term | b.trunc).bool().any(0).cpu().numpy()
    assert ended.sum() > n // 2
    first = {}
    for i, e in enumerate(rec["env"].tolist()):
        first.setdefault(e, i)
    assert sorted(first) == np.nonzero(ended)[0].tolist()
    idx = np.array([first[e] for e in sorted(first)])
    envs = np.array(sorted(first))
    assert np.array_equal(rec["length"][idx], ev["steps"][envs])
    assert np.array_equal(rec["orders_completed"][idx], ev["orders_completed"][envs])
    assert np.array_equal(rec["packaged"][idx], ev["products_packaged"][envs])
    assert rec["by_agent"][:, idx].tobytes() == np.ascontiguousarray(ev["rewards_by_agent"][:, envs]).tobytes()
    assert rec["total"][idx].tobytes() == np.ascontiguousarray(ev["total_reward"][envs]).tobytes()


# ------------------------------------------------------------------ 6. the learner
def _learner_run(M, track, fused_step=True, rounds=5):
    A, V = M["A"], M["V"]
    n, T = 128, 16
    env = V.FJSPVecEnv(n, max_episode_steps=30)
    L = A.VecMultiAgentA2C(env, batch_size=T, seed=1, track_episodes=track)
    L.fused_step = fused_step
    L.reset(seeds=torch.arange(n) + 9, num_orders=3)
    keys = ("feats", "masks", "actions", "values", "rewards", "term", "trunc", "status")
    slabs = []
    for _ in range(rounds):
        L.collect()
        if track:
            L.account_episodes()
        slabs.append({k: L._bufs[k].clone() for k in keys + (("orders_completed", "packaged")
                                                              if "orders_completed" in L._bufs else ())})
        L.update()
        L.roll_over()
    params = [p.detach().clone() for p in list(L.actors.parameters()) + list(L.critic.parameters())]
    return L, slabs, params


def _cat(slabs, k):
    return torch.cat([s[k] for s in slabs]).cpu().numpy()


@pytest.fixture(scope="module")
def tracked(M):
    return _learner_run(M, True)


def test_learner_episode_summary_equals_reference(M, tracked):
    L, slabs, _ = tracked
    n = 128
    want, _, _ = E.episodes_reference(_cat(slabs, "rewards"), _cat(slabs, "term"), _cat(slabs, "trunc"))
    rec = L.episode_summary()
    wd = E.records_dict(want)
    for k in wd:
        assert np.asarray(rec[k]).tobytes() == np.asarray(wd[k]).tobytes(), k
    assert np.bincount(rec["env"], minlength=n).min() >= 2
    assert rec["length"].max() <= 31
    assert (rec["orders_completed"] == -1).all() and (rec["packaged"] == -1).all()   # the fused collect
    assert L.overall_rewards == want["total"].tolist()
    assert L.episode_end_timesteps == (want["end_step"] * n).tolist()
    assert L.episode_summary()["total"].size == 0         # drained


def test_learner_unfused_collect_fills_the_infos(M):
    L, slabs, _ = _learner_run(M, True, fused_step=False)
    want, _, _ = E.episodes_reference(_cat(slabs, "rewards"), _cat(slabs, "term"), _cat(slabs, "trunc"),
                                      _cat(slabs, "orders_completed"), _cat(slabs, "packaged"))
    rec = L.episode_summary()
    wd = E.records_dict(want)
    for k in wd:
        assert np.asarray(rec[k]).tobytes() == np.asarray(wd[k]).tobytes(), k
    assert (rec["orders_completed"] >= 0).all() and (rec["packaged"] >= 0).all()
    assert (rec["orders_completed"][rec["terminated"]] == 3).all()


def test_tracking_does_not_perturb_training(M, tracked):
    _, slabs, params = tracked
    _, slabs0, params0 = _learner_run(M, False)
    for b, (s, s0) in enumerate(zip(slabs, slabs0)):
        for k in s0:
            assert torch.equal(s[k], s0[k]), (b, k)
    for p, p0 in zip(params, params0):
        assert torch.equal(p, p0)


def test_learn_fills_the_training_curve(M):
    A, V = M["A"], M["V"]
    n, T = 128, 16
    L = A.VecMultiAgentA2C(V.FJSPVecEnv(n, max_episode_steps=30), batch_size=T, seed=1, track_episodes=True)
    assert L.learn(5 * T * n, num_orders=3, seeds=torch.arange(n) + 9) is L
    L0, slabs, _ = _learner_run(M, True)
    rec = L0.episode_summary()
    assert len(L.overall_rewards) == len(rec["total"]) > 0
    assert L.overall_rewards == rec["total"].tolist()
    assert L.episode_end_timesteps == (rec["end_step"] * n).tolist()
    off = A.VecMultiAgentA2C(V.FJSPVecEnv(n), batch_size=T, seed=1)
    assert off.episode_log is None and off.overall_rewards == []
