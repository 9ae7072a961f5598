"""Shop-floor KPIs: per-episode scheduling metrics reduced from a rollout's full outputs.

A scheduling user judges a policy by makespan, flow times, station utilisation, queue lengths,
AGV travel and invalid actions, not by reward (whose weights are tunable).  Everything needed is
already in the step outputs: the action-result words (spec.RESULT_KEYS / RESULT_INT: the agents'
result dicts), the stations' is_busy / queue_length observations and the infos a2c.py:612-615
tracks.  ``kpi_reference`` reduces them per env in plain Python ints (the specification);
``KpiLog`` is the same scan on the device (fjsp_kpi_scan, csrc/fjsp_episode.hip), appending one
fjsp_kpi_rec per finished episode to a device-resident log with no host synchronisation until
``pop()``; ``kpi_summary`` derives the quantities a user reads from the records, on the host.

The records are numbered exactly as EpisodeLog's: scanning the same slabs into both logs from the
same starting state makes record k of each describe the same episode (equal 40-byte heads).
"""
import numpy as np

from . import _native as nat
from . import spec
from .episodes import FLAG_TERMINATED, FLAG_TRUNCATED, temp_bytes
from .slablog import EpisodeSlabLog, _ptr, word_dtypes

NA, NS = 8, 6
TIMES_DTYPE = np.dtype([("first_step", "<i4"), ("last_step", "<i4"), ("step_sum", "<i8")])
# include/fjsp.h fjsp_kpi_rec (432 bytes); the first 40 bytes are fjsp_episode_rec's
KPI_DTYPE = np.dtype([("env_gid", "<u4"), ("length", "<i4"), ("end_step", "<i8"), ("seq", "<u8"),
                      ("flags", "<i4"), ("orders_completed", "<i4"), ("packaged", "<i4"), ("reserved", "<i4"),
                      ("makespan", "<f8"), ("orders", TIMES_DTYPE), ("products", TIMES_DTYPE),
                      ("agents", "<i4", (NA, 8)), ("stations", "<i4", (NS, 4))])
assert KPI_DTYPE.itemsize == 432
HEAD_BYTES = 40
HEAD_FIELDS = ("env_gid", "length", "end_step", "seq", "flags", "orders_completed", "packaged", "reserved")
# columns of `agents`: bits 0..5 of the result word, bit 7, the sum of bits 16..31
COL_EXECUTED, COL_VALUE = 6, 7
# carry words per env (fjsp_kpi_carry_words): the open episode's counters.  The episode's steps so
# far are kept twice (C_LEN, C_LEN1: one word for each of the kernel's two waves that need them, so
# that no wave reads a word another writes); the two are always equal
C_LEN, C_TIMES, C_AGENTS, C_STATIONS, C_LEN1, CARRY_WORDS = 0, 1, 11, 75, 93, 94


def _i32(x):
    return ((int(x) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _i64(x):
    return ((int(x) + (1 << 63)) & 0xFFFFFFFFFFFFFFFF) - (1 << 63)


def _fresh():
    return {"len": 0, "times": [[0, 0, 0, 0], [0, 0, 0, 0]],          # first, last, step_sum, previous value
            "agents": [[0] * 8 for _ in range(NA)], "stations": [[0, 0, 0] for _ in range(NS)]}


def _from_carry(col):
    s = _fresh()
    s["len"] = int(col[C_LEN])
    for i in range(2):
        w = [int(x) for x in col[C_TIMES + 5 * i: C_TIMES + 5 * i + 5]]
        s["times"][i] = [w[0], w[1], _i64((w[2] & 0xFFFFFFFF) | ((w[3] & 0xFFFFFFFF) << 32)), w[4]]
    for a in range(NA):
        s["agents"][a] = [int(x) for x in col[C_AGENTS + 8 * a: C_AGENTS + 8 * a + 8]]
    for k in range(NS):
        s["stations"][k] = [int(x) for x in col[C_STATIONS + 3 * k: C_STATIONS + 3 * k + 3]]
    return s


def _to_carry(s):
    col = [0] * CARRY_WORDS
    col[C_LEN] = col[C_LEN1] = s["len"]
    for i in range(2):
        first, last, ssum, prev = s["times"][i]
        col[C_TIMES + 5 * i: C_TIMES + 5 * i + 5] = [first, last, _i32(ssum & 0xFFFFFFFF), _i32((ssum >> 32) & 0xFFFFFFFF),
                                                     prev]
    for a in range(NA):
        col[C_AGENTS + 8 * a: C_AGENTS + 8 * a + 8] = s["agents"][a]
    for k in range(NS):
        col[C_STATIONS + 3 * k: C_STATIONS + 3 * k + 3] = s["stations"][k]
    return col


def kpi_reference(results, term, trunc, obs_i8=None, orders_completed=None, packaged=None, sim_time=None,
                  carry=None, step0=0, env_gid0=0, seq0=0):
    """The specification of fjsp_kpi_scan on the host.  results [T, 8, N] (the 32-bit result words,
    any integer dtype; None: agent blocks of 0), term / trunc [T, N], optional obs_i8 [T, 12, N],
    orders_completed / packaged [T, N], sim_time [T, N] (f64); carry int32 [CARRY_WORDS, N] = the
    open episodes' counters (None: fresh).  Returns (records, carry): records a KPI_DTYPE array in
    (t, e) order, numbered from seq0, and the carry after the slab.

    One env at a time, Python ints: per step l (1-based within the episode) every agent's result
    bits are counted and its value summed, every station's post-step is_busy / queue_length
    reduced, and a rise d > 0 of an infos counter noted at l (first, last, sum of d * l).  A slab
    that is None counts as all zeros for this call's rows (so a block whose slab is never given is
    all 0, and a counter's previous value is 0 after a call without its slab); the head's
    orders_completed / packaged / makespan of the records this call writes are then -1 / NaN."""
    term = np.asarray(term)
    T, N = term.shape
    trunc = np.asarray(trunc).reshape(T, N)
    res = None
    if results is not None:
        res = (np.asarray(results).astype(np.int64) & 0xFFFFFFFF).reshape(T, NA, N)
    obs = None if obs_i8 is None else np.asarray(obs_i8).astype(np.int8).reshape(T, 2 * NS, N)
    infos = [None if x is None else np.asarray(x).reshape(T, N) for x in (orders_completed, packaged)]
    st = None if sim_time is None else np.asarray(sim_time, dtype=np.float64).reshape(T, N)
    states = [_fresh() if carry is None else _from_carry(np.asarray(carry)[:, e]) for e in range(N)]
    ends = []   # (t, e, record): sorted into (t, e) order at the end, the order the kernel numbers them in
    for e in range(N):
        s = states[e]
        for t in range(T):
            s["len"] += 1
            ln = s["len"]
            if res is not None:
                for a in range(NA):
                    w = int(res[t, a, e])
                    c = s["agents"][a]
                    for k in range(6):
                        c[k] = _i32(c[k] + ((w >> k) & 1))
                    c[COL_EXECUTED] = _i32(c[COL_EXECUTED] + ((w >> 7) & 1))
                    c[COL_VALUE] = _i32(c[COL_VALUE] + (w >> 16))
            if obs is not None:
                for k in range(NS):
                    busy, q = int(obs[t, 2 * k, e]), int(obs[t, 2 * k + 1, e])
                    z = s["stations"][k]
                    z[0] = _i32(z[0] + (1 if busy != 0 else 0))
                    z[1] = _i32(z[1] + q)
                    z[2] = max(z[2], q)
            else:
                for z in s["stations"]:
                    z[2] = max(z[2], 0)   # zeros: only a negative carried maximum could change
            for i in range(2):
                v = 0 if infos[i] is None else int(infos[i][t, e])   # a slab not given counts as zeros
                tm = s["times"][i]
                d = v - tm[3]
                if d > 0:
                    if tm[0] == 0:
                        tm[0] = ln
                    tm[1] = ln
                    tm[2] = _i64(tm[2] + d * ln)
                tm[3] = v
            te, tr = int(term[t, e]) != 0, int(trunc[t, e]) != 0
            if te or tr:
                ends.append((t, e, (
                    env_gid0 + e, ln, step0 + t + 1, 0,
                    (FLAG_TERMINATED if te else 0) | (FLAG_TRUNCATED if tr else 0),
                    -1 if infos[0] is None else int(infos[0][t, e]), -1 if infos[1] is None else int(infos[1][t, e]),
                    0, float("nan") if st is None else float(st[t, e]),
                    tuple(s["times"][0][:3]), tuple(s["times"][1][:3]),
                    [list(c) for c in s["agents"]], [list(z) + [0] for z in s["stations"]])))
                s = states[e] = _fresh()
    ends.sort(key=lambda x: (x[0], x[1]))
    recs = np.zeros(len(ends), dtype=KPI_DTYPE)
    for k, (_, _, r) in enumerate(ends):
        recs[k] = r
    recs["seq"] = seq0 + np.arange(len(ends), dtype=np.uint64)
    out = np.array([_to_carry(s) for s in states], dtype=np.int64).astype(np.int32).T.copy() if N else \
        np.zeros((CARRY_WORDS, 0), np.int32)
    return recs, out


def records_dict(recs, dropped=0):
    """KPI_DTYPE array -> the dict of arrays KpiLog.pop() returns."""
    d = {"env": recs["env_gid"].copy(), "length": recs["length"].copy(), "end_step": recs["end_step"].copy(),
         "seq": recs["seq"].copy(), "terminated": (recs["flags"] & FLAG_TERMINATED) != 0,
         "truncated": (recs["flags"] & FLAG_TRUNCATED) != 0, "orders_completed": recs["orders_completed"].copy(),
         "packaged": recs["packaged"].copy(), "makespan": recs["makespan"].copy()}
    for name in ("orders", "products"):
        for f in TIMES_DTYPE.names:
            d[f"{name}_{f}"] = recs[name][f].copy()
    d["agents"] = np.ascontiguousarray(recs["agents"].transpose(1, 2, 0))       # [8 agents, 8 columns, n]
    d["stations"] = np.ascontiguousarray(recs["stations"].transpose(1, 2, 0))   # [6, 4, n]
    d["records"] = recs
    d["dropped"] = int(dropped)
    return d


def result_column(agent, key):
    """Column of `agents[a]` holding the reference's result key `key` of agent `agent`
    (spec.RESULT_KEYS bit order; RESULT_INT's value; 'executed')."""
    kind = spec.agent_kind(agent)
    if key == "executed":
        return COL_EXECUTED
    if spec.RESULT_INT.get(kind) == key:
        return COL_VALUE
    return spec.RESULT_KEYS[kind].index(key)


def kpi_summary(records, config=None):
    """Per-episode derived quantities of KPI records (a KPI_DTYPE array or KpiLog.pop()'s dict) as
    a dict of numpy arrays, n = the number of records.  config: an fjsp_config (or anything with
    step_size; None = the default config) for the step -> time conversion.

    makespan [n]; mean_order_flow_time / mean_product_flow_time [n] = step_sum / completed *
    step_size (every order is in the queue at reset; NaN where none completed); utilisation [6, n]
    = busy_steps / length; mean_queue [6, n]; queue_max [6, n]; agv_distance [n];
    agv_invalid_rate [n] = invalid actions / length; idle_with_work [8, n] = steps an agent idled
    with work waiting (idle_with_orders / idle_with_queue; 0 for the AGV)."""
    recs = records["records"] if isinstance(records, dict) else np.asarray(records)
    if config is None:
        step_size = nat.default_config().step_size
    else:
        step_size = config["step_size"] if isinstance(config, dict) else config.step_size
    n = len(recs)
    length = recs["length"].astype(np.float64)

    def flow(block, completed):
        c = recs[completed].astype(np.float64)
        out = np.full(n, np.nan)
        ok = c > 0
        out[ok] = recs[block]["step_sum"][ok].astype(np.float64) / c[ok] * float(step_size)
        return out
    stations = recs["stations"].astype(np.float64)            # [n, 6, 4]
    agents = recs["agents"]
    agv = spec.AGENTS.index("agv")
    idle = np.zeros((NA, n), dtype=np.int64)
    for a, name in enumerate(spec.AGENTS):
        keys = spec.RESULT_KEYS[spec.agent_kind(name)]
        for k in ("idle_with_orders", "idle_with_queue"):
            if k in keys:
                idle[a] = agents[:, a, keys.index(k)]
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"makespan": recs["makespan"].copy(),
                "mean_order_flow_time": flow("orders", "orders_completed"),
                "mean_product_flow_time": flow("products", "packaged"),
                "utilisation": (stations[:, :, 0] / length[:, None]).T.copy(),
                "mean_queue": (stations[:, :, 1] / length[:, None]).T.copy(),
                "queue_max": recs["stations"][:, :, 2].T.copy(),
                "agv_distance": agents[:, agv, result_column("agv", "distance")].copy(),
                "agv_invalid_rate": agents[:, agv, result_column("agv", "invalid_action")] / length,
                "idle_with_work": idle}


def best_of(records, samples, instances=None, env_id_base=0):
    """Best-of-K selection over KPI records (a KPI_DTYPE array or KpiLog.pop()'s dict) of a run in
    which env i * samples + r is replica r of instance i (FJSPVecEnv.solve).  Only each env's first
    episode counts (end_step == length).  Per instance the terminated replica of least makespan
    wins, ties going to the lowest env; if no replica terminated the winner is the one with the
    most orders_completed, then the most packaged, then the lowest env, and the instance is not
    solved.  instances: their number (None: as many as the records' highest env needs).

    Returns best_env [I] (env index, without env_id_base), solved [I], makespan [I] (NaN where
    unsolved), all_makespans [I, samples] (NaN where the replica did not terminate), index [I]
    (the winner's row in `records`, -1 if it finished no episode) and records [I] (the winners'
    records; zeros where index is -1).  Needs no GPU."""
    recs = records["records"] if isinstance(records, dict) else np.asarray(records)
    samples = int(samples)
    if samples < 1:
        raise ValueError("samples must be at least 1")
    first = np.flatnonzero(recs["end_step"] == recs["length"])
    env = recs["env_gid"][first].astype(np.int64) - int(env_id_base)
    if instances is None:
        instances = int(-(-(env.max() + 1) // samples)) if len(env) else 0
    I = int(instances)
    if len(env) and (env.min() < 0 or env.max() >= I * samples):
        raise ValueError("a record's env lies outside instances * samples")
    if len(np.unique(env)) != len(env):
        raise ValueError("two first episodes of one env")
    row = np.full(I * samples, -1, np.int64)
    row[env] = first
    have = row >= 0
    term = np.zeros(I * samples, bool)
    term[have] = (recs["flags"][row[have]] & FLAG_TERMINATED) != 0
    span = np.full(I * samples, np.nan)
    span[term] = recs["makespan"][row[term]]
    done = np.full(I * samples, -1, np.int64)
    packed = np.full(I * samples, -1, np.int64)
    done[have], packed[have] = recs["orders_completed"][row[have]], recs["packaged"][row[have]]
    span, term, done, packed = (x.reshape(I, samples) for x in (span, term, done, packed))
    solved = term.any(axis=1)
    best = np.zeros(I, np.int64)
    for i in range(I):
        if solved[i]:
            best[i] = int(np.argmin(np.where(term[i], span[i], np.inf)))        # the first of equal minima
        else:
            best[i] = min(range(samples), key=lambda r: (-done[i, r], -packed[i, r], r))
    best_env = np.arange(I) * samples + best
    index = row[best_env] if I else np.zeros(0, np.int64)
    winners = np.zeros(I, dtype=recs.dtype)
    winners[index >= 0] = recs[index[index >= 0]]
    return {"best_env": best_env, "solved": solved, "makespan": np.where(solved, span[np.arange(I), best], np.nan),
            "all_makespans": span, "index": index, "records": winners}


def carry_words():
    return int(nat.lib().fjsp_kpi_carry_words())


class KpiLog(EpisodeSlabLog):
    """Device-resident KPI log of num_envs envs: the carry of the open episodes (their counters so
    far), a record buffer of `capacity` fjsp_kpi_rec, the device-side episode count and the
    running vector-step counter step0.  scan() appends without synchronising; pop() copies the
    records to the host (the only synchronisation) and empties the log."""
    REC_DTYPE = KPI_DTYPE

    def __init__(self, num_envs, device, capacity=65536, env_id_base=0):
        import torch
        super().__init__(num_envs, device, capacity, env_id_base)
        words = carry_words()
        assert words == CARRY_WORDS, (words, CARRY_WORDS)
        self.carry = torch.zeros(words, self.N, dtype=torch.int32, device=self.device)

    def _temp_bytes(self, T):
        return temp_bytes(T, self.N)

    def scan(self, results, term, trunc, obs_i8=None, orders_completed=None, packaged=None, sim_time=None):
        """Reduce the slab (contiguous device tensors: results int32 / uint32 [T, 8, N], term / trunc
        u8 [T, N], obs_i8 int8 [T, 12, N], int32 infos slabs [T, N], sim_time f64 [T, N]; every one
        but term / trunc may be None) on the current stream; advances step0 by T."""
        import torch
        T, N = int(term.shape[0]), self.N
        self._launch(T, (("results", results, word_dtypes(), (T, NA, N), False),
                         ("term", term, (torch.uint8,), (T, N), True),
                         ("trunc", trunc, (torch.uint8,), (T, N), True),
                         ("obs_i8", obs_i8, (torch.int8,), (T, 2 * NS, N), False),
                         ("orders_completed", orders_completed, (torch.int32,), (T, N), False),
                         ("packaged", packaged, (torch.int32,), (T, N), False),
                         ("sim_time", sim_time, (torch.float64,), (T, N), False)),
                     lambda temp, nbytes, stream: nat.lib().fjsp_kpi_scan(
                         _ptr(results), _ptr(term), _ptr(trunc), _ptr(obs_i8), _ptr(orders_completed), _ptr(packaged),
                         _ptr(sim_time), T, N, self.env_id_base, self.step0, _ptr(self.carry), _ptr(self.recs),
                         self.capacity, _ptr(self.count), temp, nbytes, stream))

    def pop(self):
        """Every record logged since the last pop, in seq order, as a dict of numpy arrays: the head
        (env, length, end_step, seq, terminated, truncated, orders_completed, packaged), makespan,
        orders_* / products_* (first_step, last_step, step_sum), agents [8, 8, n], stations
        [6, 4, n], the raw `records` and dropped = the episodes that did not fit the capacity.
        Synchronises; empties the log (the carry of the open episodes is kept)."""
        return records_dict(*self.pop_records())


__all__ = ["kpi_reference", "kpi_summary", "KpiLog", "KPI_DTYPE", "TIMES_DTYPE", "HEAD_BYTES", "HEAD_FIELDS",
           "CARRY_WORDS", "records_dict", "result_column", "carry_words", "best_of"]
