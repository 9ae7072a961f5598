"""Shop-floor KPIs on the GPU (fjsp_kpi_scan, kpis.KpiLog) against kpi_reference, the plain-Python
specification, byte for byte on every field: the reference's recorded traces through the kernel
with every optional slab given or NULL, synthetic edge slabs, the capacity bound, appending
without synchronisation, the join with the episode log, FJSPVecEnv.evaluate_kpis and the
learners' evaluate_kpis."""
import ctypes
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from tests import episodes_util as U  # noqa: E402
from tests import kpi_util as KU  # noqa: E402

E = U.episodes
K = KU.kpis


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from tests import gpu_util  # noqa: F401
    return {"A": importlib.import_module("multi-agent-rl-for-fjsp_amd.a2c_vec"),
            "P": importlib.import_module("multi-agent-rl-for-fjsp_amd.ppo_vec"),
            "V": importlib.import_module("multi-agent-rl-for-fjsp_amd.vec_env"),
            "nat": importlib.import_module("multi-agent-rl-for-fjsp_amd._native")}


def _dev(slab, given=KU.OPTIONAL):
    """KpiLog.scan's arguments on the device; the optional slabs not in `given` are None."""
    d = {k: torch.from_numpy(np.array(slab[k])).cuda() for k in KU.KEYS if k in ("term", "trunc") or k in given}
    return tuple(d.get(k) for k in KU.KEYS)


def _results_i32(slab):
    s = dict(slab)
    s["results"] = np.ascontiguousarray(slab["results"]).view(np.int32)
    return s


def _scan_split(log, slab, rows, given=KU.OPTIONAL):
    T = slab["term"].shape[0]
    slab = _results_i32(slab)
    for lo, hi in U.cuts(T, rows):
        log.scan(*_dev(U.rows_of(slab, lo, hi), given))


# ------------------------------------------------------------------ 1. golden replay
@pytest.mark.parametrize("given", ["all", "none", "results", "no_results"])
@pytest.mark.parametrize("rows", (1000,) + U.SPLITS)
def test_golden_traces_through_the_kernel(M, rows, given):
    slab = KU.trace_slab()
    want, carry = KU.trace_reference(KU.GIVEN[given])
    assert len(want) == 71
    log = K.KpiLog(12, "cuda", capacity=128)
    _scan_split(log, slab, rows, KU.GIVEN[given])
    got, dropped = log.pop_records()
    assert dropped == 0
    KU.same(got, want)
    assert log.carry.cpu().numpy().tobytes() == carry.tobytes()
    assert log.step0 == 1000


# ------------------------------------------------------------------ 2. ordering and edges
@pytest.mark.parametrize("N", [130, 1, 64])
def test_synthetic_ordering_and_edges(M, N):
    slab = KU.synthetic_slab(N)
    want, carry = KU.reference(slab, env_gid0=1000, step0=0)
    done = (slab["term"] | slab["trunc"]).astype(bool)
    assert not done[5].any() and done[11].all() and done[0].any() and done[-1].any()
    flags = set(want["flags"].tolist())
    assert flags == {1, 2, 3} or N == 1
    w = slab["results"]
    assert all(((w >> k) & 1).any() for k in (0, 1, 2, 3, 4, 5, 7)) and (w >> 16).any()
    assert (np.diff(slab["orders_completed"].astype(np.int64), axis=0) < 0).any()
    log = K.KpiLog(N, "cuda", capacity=len(want) + 3, env_id_base=1000)
    log.scan(*_dev(_results_i32(slab)))
    got, dropped = log.pop_records()
    assert dropped == 0
    KU.same(got, want)
    assert log.carry.cpu().numpy().tobytes() == carry.tobytes()
    # a second slab continues the open episodes from the carry
    want2, carry2 = KU.reference(slab, carry=carry, step0=37, env_gid0=1000, seq0=len(want))
    log.scan(*_dev(_results_i32(slab)))
    KU.same(log.pop_records()[0], want2)
    assert log.carry.cpu().numpy().tobytes() == carry2.tobytes()


# ------------------------------------------------------------------ 3. capacity
def test_capacity_bounds_the_writes(M):
    nat = M["nat"]
    N, cap, guard = 130, 5, 64
    slab = KU.synthetic_slab(N)
    want, _ = KU.reference(slab)
    assert len(want) > cap + guard
    T = slab["term"].shape[0]
    size = K.KPI_DTYPE.itemsize
    buf = torch.full(((cap + guard) * size,), 0xA5, dtype=torch.uint8, device="cuda")
    carry = torch.zeros(K.CARRY_WORDS, N, dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    temp = torch.empty(E.temp_bytes(T, N), dtype=torch.uint8, device="cuda")
    args = _dev(_results_i32(slab))
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    nat.check(nat.lib().fjsp_kpi_scan(*[P(x) for x in args], T, N, 0, 0, P(carry), P(buf), cap, P(count), P(temp),
                                      temp.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    raw = buf.cpu().numpy()
    assert int(count.item()) == len(want) > cap
    KU.same(raw[:cap * size].view(K.KPI_DTYPE), want[:cap])
    assert (raw[cap * size:] == 0xA5).all()
    # the same through the log: pop() reports what did not fit
    log = K.KpiLog(N, "cuda", capacity=cap)
    log.scan(*args)
    got = log.pop()
    assert got["dropped"] == len(want) - cap and len(got["makespan"]) == cap
    KU.same(got["records"], want[:cap])
    # cap == 0 with no record buffer: only the count advances
    count.zero_()
    carry.zero_()
    nat.check(nat.lib().fjsp_kpi_scan(*[P(x) for x in args], T, N, 0, 0, P(carry), None, 0, P(count), P(temp),
                                      temp.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert int(count.item()) == len(want)


# ------------------------------------------------------------------ 4. append without sync
def test_two_scans_append_with_no_synchronising_torch_call(M):
    """Two scans in a row append to one log.  What a test can observe of "no host synchronisation":
    torch's sync debug mode raises on any synchronising torch call (.item(), .cpu(), ...) while
    the two scans run; the C entry itself only launches (it has no synchronising HIP call to
    observe from here)."""
    N = 130
    a, b = KU.synthetic_slab(N), KU.synthetic_slab(N, seed=77)
    both = {k: np.concatenate([a[k], b[k]]) for k in a}
    want, _ = KU.reference(both)
    log = K.KpiLog(N, "cuda", capacity=len(want))
    da, db = _dev(_results_i32(a)), _dev(_results_i32(b))
    log._temp_for(37)                  # allocated once, as in a running loop
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        log.scan(*da)
        log.scan(*db)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    got, dropped = log.pop_records()
    assert dropped == 0
    assert got["seq"].tolist() == list(range(len(want)))
    KU.same(got, want)


@pytest.mark.parametrize("N", [130, 1])
def test_given_slabs_may_change_between_calls(M, N):
    """An episode open across calls of which only some give a slab: a slab not given counts as
    zeros for that call's rows, in the kernel as in the specification (records and carry)."""
    a, b = KU.synthetic_slab(N), KU.synthetic_slab(N, seed=77)
    log = K.KpiLog(N, "cuda", capacity=4096)
    carry, want, step0 = None, [], 0
    for slab, given in ((a, "all"), (b, "none"), (a, "results"), (b, "no_results"), (a, "all")):
        r, carry = KU.reference(slab, KU.GIVEN[given], carry=carry, step0=step0, seq0=sum(len(x) for x in want))
        want.append(r)
        step0 += 37
        log.scan(*_dev(_results_i32(slab), KU.GIVEN[given]))
        assert log.carry.cpu().numpy().tobytes() == carry.tobytes(), given
    got, dropped = log.pop_records()
    assert dropped == 0
    KU.same(got, np.concatenate(want))
    c = log.carry.cpu().numpy()
    assert (c[K.C_LEN] == c[K.C_LEN1]).all()


# ------------------------------------------------------------------ 5. the join with the episode log
def test_kpi_and_episode_records_join_by_index(M):
    N = 130
    a, b = KU.synthetic_slab(N), KU.synthetic_slab(N, seed=77)
    ep = E.EpisodeLog(N, "cuda", capacity=4096, env_id_base=50)
    kp = K.KpiLog(N, "cuda", capacity=4096, env_id_base=50)
    for s in (a, b):
        r = torch.from_numpy(np.array(s["rewards"])).cuda()
        args = _dev(_results_i32(s))
        ep.scan(r, args[1], args[2], args[4], args[5])
        kp.scan(*args)
    er, ed = ep.pop_records()
    kr, kd = kp.pop_records()
    assert ed == kd == 0 and len(er) == len(kr) > 2 * N
    assert KU.heads(er).tobytes() == KU.heads(kr).tobytes()
    for i in (0, len(er) // 2, len(er) - 1):
        assert KU.heads(er[i:i + 1]).tobytes() == KU.heads(kr[i:i + 1]).tobytes()
    # and on the recorded traces
    slab = KU.trace_slab()
    ep, kp = E.EpisodeLog(12, "cuda", capacity=128), K.KpiLog(12, "cuda", capacity=128)
    for lo, hi in U.cuts(1000, 256):
        part = _results_i32(U.rows_of(slab, lo, hi))
        args = _dev(part)
        ep.scan(torch.from_numpy(np.array(part["rewards"])).cuda(), args[1], args[2], args[4], args[5])
        kp.scan(*args)
    er, kr = ep.pop_records()[0], kp.pop_records()[0]
    assert len(er) == len(kr) == 71 and KU.heads(er).tobytes() == KU.heads(kr).tobytes()


# ------------------------------------------------------------------ 6. on the env
def _first_records(env_ids):
    first = {}
    for i, e in enumerate(env_ids.tolist()):
        first.setdefault(e, i)
    return first


def test_evaluate_kpis_on_the_env(M):
    V = M["V"]
    n, steps, chunk = 130, 300, 64
    seeds = torch.arange(n) * 5 + 2
    got = V.FJSPVecEnv(n).evaluate_kpis("heuristic", num_orders=5, steps=steps, seeds=seeds, chunk=chunk)
    eps = V.FJSPVecEnv(n).evaluate_episodes("heuristic", num_orders=5, steps=steps, seeds=seeds, chunk=chunk)
    assert sorted(got) == ["episodes", "kpis"] and sorted(got["episodes"]) == sorted(eps)
    for k in eps:
        assert np.asarray(got["episodes"][k]).tobytes() == np.asarray(eps[k]).tobytes(), k
    # a second, identical run through rollout, its slabs kept
    env = V.FJSPVecEnv(n)
    env.reset(seeds=seeds, num_orders=5)
    keep = []
    for lo, hi in U.cuts(steps, chunk):
        b = env.rollout(hi - lo, step0=lo, policy="heuristic", autoreset=True, infos=True)
        keep.append({k: getattr(b, k).cpu().numpy() for k in KU.KEYS})
    slab = {k: np.concatenate([s[k] for s in keep]) for k in keep[0]}
    want, _ = KU.reference(slab)
    kp = got["kpis"]
    assert kp["dropped"] == 0 and len(want) >= n
    KU.same(kp["records"], want)
    assert KU.heads(kp["records"]).shape == (len(eps["total"]), 40)
    assert np.array_equal(kp["env"], eps["env"]) and np.array_equal(kp["length"], eps["length"])
    assert (kp["makespan"] == kp["length"] * 10.0).all()
    # each env's first record agrees with evaluate()
    ev = V.FJSPVecEnv(n).evaluate("heuristic", num_orders=5, max_steps=steps, seeds=seeds)
    first = _first_records(kp["env"])
    assert len(first) > n // 2
    envs = np.array(sorted(first))
    idx = np.array([first[e] for e in envs])
    assert np.array_equal(kp["length"][idx], ev["steps"][envs])
    assert np.array_equal(kp["orders_completed"][idx], ev["orders_completed"][envs])
    assert np.array_equal(kp["packaged"][idx], ev["products_packaged"][envs])
    s = K.kpi_summary(kp, env.config)
    assert s["utilisation"].shape == (6, len(want)) and (s["utilisation"] <= 1.0).all()


# ------------------------------------------------------------------ 7. the learners
def _check_learner_result(res, n):
    tr = res["trace"]
    want, _ = K.kpi_reference(tr["results"], tr["term"], tr["trunc"], tr["obs_i8"], tr["orders_completed"],
                              tr["packaged"], tr["sim_time"])
    assert res["kpis"]["dropped"] == 0 and len(want) >= n
    KU.same(res["kpis"]["records"], want)
    ew, _, _ = E.episodes_reference(tr["rewards"], tr["term"], tr["trunc"], tr["orders_completed"], tr["packaged"])
    wd = E.records_dict(ew)
    for k in wd:
        assert np.asarray(res["episodes"][k]).tobytes() == np.asarray(wd[k]).tobytes(), k
    return want


def _losses(x):
    al, cl = x
    return np.asarray(al, dtype=np.float64).ravel().tolist() + np.asarray(cl, dtype=np.float64).ravel().tolist()


def _train_once(M, cls, with_eval):
    V = M["V"]
    n, T = 66, 16
    L = cls(V.FJSPVecEnv(n, max_episode_steps=30), batch_size=T, seed=1)
    L.reset(seeds=torch.arange(n) + 9, num_orders=3)
    res = None
    if with_eval:
        res = L.evaluate_kpis(num_orders=5, steps=256, seeds=torch.arange(n) * 3 + 1, env=V.FJSPVecEnv(n), chunk=64,
                              trace=True)
    L.collect()
    return L, res, _losses(L.update())


def test_learner_evaluate_kpis(M):
    A, V = M["A"], M["V"]
    n = 66
    L, res, losses = _train_once(M, A.VecMultiAgentA2C, True)
    want = _check_learner_result(res, n)
    assert res["trace"]["actions"].shape == (256, 8, n)
    # each env's first episode agrees with test() from the same seeds
    t = L.test(num_orders=5, max_steps=256, seeds=torch.arange(n) * 3 + 1, deterministic=True, env=V.FJSPVecEnv(n))
    first = _first_records(want["env_gid"])
    assert sorted(first) == list(range(n))          # every env ends an episode within 256 steps (truncation at 200)
    idx = np.array([first[e] for e in range(n)])
    assert np.array_equal(want["length"][idx], t["steps"])
    assert np.array_equal(want["orders_completed"][idx], t["orders_completed"])
    assert np.array_equal(want["packaged"][idx], t["products_packaged"])
    # training state untouched: the same losses as a learner that never evaluated
    _, _, losses0 = _train_once(M, A.VecMultiAgentA2C, False)
    assert losses == losses0


def test_learner_evaluate_kpis_on_the_training_env_and_ppo(M):
    P, V = M["P"], M["V"]
    n, T = 66, 16
    L = P.VecMultiAgentPPO(V.FJSPVecEnv(n, max_episode_steps=30), batch_size=T, seed=1)
    L.reset(seeds=torch.arange(n) + 9, num_orders=3)
    res = L.evaluate_kpis(num_orders=2, steps=70, seeds=torch.arange(n), chunk=64, trace=True)
    want = _check_learner_result(res, n)
    assert want["length"].max() <= 31 and res["trace"]["term"].shape == (70, n)
    view = L.env.read_env(0)                                 # restored as test() does: a fresh training episode
    assert L.num_orders == 3 and view.num_orders == 3 and view.current_step == 0
    L.collect()
    al, cl = L.update()
    assert all(np.isfinite(v) for v in _losses((al, cl)))
