"""Per-operation schedules: which tray of which order was on which machine from when to when, and
what the AGV carried from where to where (the data of a Gantt chart).

The reference shows this through its logger and grid view (utils/Logger.py processing_start /
tray_pickup / tray_drop, visualization.py).  Here a step emits three held-tray words per env
(fjsp_step_held: the AGV's carrying_tray and position, the machines' current_tray and is_busy)
beside the action-result words, and a scan compacts the per-step rows into one record per
operation.  ``schedule_reference`` is that scan in plain Python ints (the specification, usable on
numpy arrays and CPU tensors); ``ScheduleLog`` is the same scan on the device
(fjsp_schedule_scan, csrc/fjsp_episode.hip), appending fjsp_op_rec records to a device-resident
log with no host synchronisation until ``pop()``; ``gantt`` and ``check`` work on the records.

Rules, per env and row, s = the 0-based step within the episode, resources in the order AGV, small
machine, big machine:
  machine   result bit 1 (started_processing) opens an op with the row's held code, start = s; then
            an open op whose held busy bit is 0 closes with end = s (the completion due at time
            s * step_size fires in that row's run, so (end - start) * step_size = count * pt; an
            empty tray gives end == start)
  AGV       result bit 3 (pickup_success) opens an op with the held code, from = the held location;
            result bit 4 (drop_success) closes it with to = the held location
  episode end (term | trunc)  after the row's closes every op still open is written unfinished
            (finished = 0, end = -1, AGV to = 0)
A record's (env, episode_start) equals an EpisodeLog / KpiLog record's (env, end_step - length).


Packaging runs (agents 4..7; the reference's logger events packaging_start / packaging_complete).
One START grants a whole queue of tray runs of several orders and batches overlap, but per station
the runs are FIFO: arrival order = grant order = completion order.  fjsp_step_sched stores four
pack words per env beside the held words (``pack_fields``: runs, pending, completed of each
station), and ``packaging_reference`` / ``PackagingLog`` (fjsp_packaging_scan) turn them into one
record per tray run, the same 32-byte record with resource 4 + station.  Rules, per env and row,
ln = the step within the episode, prev_s = station s's pack word and Hprev = the AGV's held word of
the episode's previous row (0 at its first):
  arrival     the AGV's result has drop_success and delivered_to_packaging (bits 4, 5) and pending +
              completed of s rose against prev_s: a run with code Hprev & HELD_CODE_MASK joins the
              tail of s's FIFO, ungranted (a drop whose products are lost raises no counter)
  start       result bit 1 of agent 4 + s (started_packaging) grants every ungranted run of the
              FIFO, the one that arrived in this row included, with start = ln
  completion  runs(prev_s) + arrived - runs(now) runs leave the FIFO's head, finished, end = ln
              (taken from the FIFO's own length, which is runs(prev_s) whenever the scan saw the
              episode from its first row)
  episode end after the completions every run left is written in FIFO order, unfinished: granted
              runs keep their start and get end = -1, ungranted ones get start = end = -1
``check_packaging`` checks the records, ``arrivals`` joins them to the AGV's drops (start - arrival
is the wait in the station's queue), and ``gantt`` takes them as they are.

Not covered: the pickup station's tray release times, the fused and training step paths,
multi-GPU aggregation of the logs.
"""
import ctypes

import numpy as np

from . import _native as nat
from .slablog import SlabLog, _ptr, word_dtypes

# include/fjsp.h fjsp_op_rec (32 bytes)
OP_DTYPE = np.dtype([("env_gid", "<u4"), ("info", "<u4"), ("episode_start", "<i8"), ("tray", "<u4"),
                     ("start", "<i4"), ("end", "<i4"), ("reserved", "<i4")])
assert OP_DTYPE.itemsize == 32
HELD_ROWS = 3                       # AGV, small machine, big machine = agents 1..3
HELD_CODE_MASK, HELD_HOLDS, HELD_BUSY, HELD_LOC_SHIFT = 0x1FFF, 0x2000, 0x4000, 16
RES_AGV_PICKUP, RES_AGV_DROP, RES_MACHINE_START = 1 << 3, 1 << 4, 1 << 1   # spec.RESULT_KEYS bit order
RESOURCES = ("agv", "small_machine", "big_machine")                          # resource = 1 + index
MACHINE_LOC = (0, 3, 2)             # LocationType: SMALL_MACHINE = 3, BIG_MACHINE = 2
INFO_FINISHED = 1 << 8
# carry words per env (fjsp_schedule_carry_words): the open episode's length, then per resource the
# open op's word (open bit 0 | tray code [1,14) | from [16,20)) and its start step
C_LEN, C_OP, CARRY_WORDS = 0, 1, 7
NA = 8


def tray_fields(code):
    """(order, first product, count) of a tray code (array or int)."""
    c = np.asarray(code).astype(np.int64)
    return c & 63, (c >> 6) & 15, (c >> 10) & 7


def schedule_reference(results, held, term, trunc, carry=None, step0=0, env_gid0=0):
    """The specification of fjsp_schedule_scan on the host.  results [T, 8, N] (the 32-bit result
    words, any integer dtype), held [T, 3, N], term / trunc [T, N]; carry int32 [CARRY_WORDS, N] =
    the open episodes' state (None: fresh).  Returns (records, carry): records an OP_DTYPE array in
    (t, env, resource) order and the carry after the slab."""
    term = np.asarray(term)
    T, N = term.shape
    trunc = np.asarray(trunc).reshape(T, N)
    res = (np.asarray(results).astype(np.int64) & 0xFFFFFFFF).reshape(T, NA, N)
    hld = (np.asarray(held).astype(np.int64) & 0xFFFFFFFF).reshape(T, HELD_ROWS, N)
    cy = np.zeros((CARRY_WORDS, N), np.int64) if carry is None else np.asarray(carry).astype(np.int64).copy()
    out = []
    for e in range(N):
        ln = int(cy[C_LEN, e])
        op = [int(cy[C_OP + 2 * r, e]) & 0xFFFFFFFF for r in range(HELD_ROWS)]
        st = [int(cy[C_OP + 2 * r + 1, e]) for r in range(HELD_ROWS)]
        for t in range(T):
            end = bool(term[t, e]) or bool(trunc[t, e])
            for r in range(HELD_ROWS):
                rw, hw = int(res[t, 1 + r, e]), int(hld[t, r, e])
                loc = (hw >> HELD_LOC_SHIFT) & 7 if r == 0 else MACHINE_LOC[r]
                if rw & (RES_AGV_PICKUP if r == 0 else RES_MACHINE_START):
                    op[r] = 1 | ((hw & HELD_CODE_MASK) << 1) | (loc << 16)
                    st[r] = ln
                if not op[r] & 1:
                    continue
                fin = bool(rw & RES_AGV_DROP) if r == 0 else not hw & HELD_BUSY
                if fin or end:
                    frm = (op[r] >> 16) & 15
                    to = (loc if fin else 0) if r == 0 else frm
                    info = (1 + r) | (INFO_FINISHED if fin else 0) | (frm << 16) | (to << 20)
                    out.append((t, e, r, (env_gid0 + e, info, step0 + t - ln, (op[r] >> 1) & HELD_CODE_MASK,
                                          st[r], ln if fin else -1, 0)))
                    op[r], st[r] = 0, 0
            ln = 0 if end else ln + 1
        cy[C_LEN, e] = ln
        for r in range(HELD_ROWS):
            cy[C_OP + 2 * r, e], cy[C_OP + 2 * r + 1, e] = op[r], st[r]
    out.sort(key=lambda x: x[:3])
    recs = np.zeros(len(out), dtype=OP_DTYPE)
    for k, x in enumerate(out):
        recs[k] = x[3]
    return recs, cy.astype(np.int32)


def records_dict(recs, dropped=0):
    """OP_DTYPE array -> the dict of arrays ScheduleLog.pop() returns."""
    info = recs["info"].astype(np.int64)
    order, first, count = tray_fields(recs["tray"])
    return {"env": recs["env_gid"].copy(), "episode_start": recs["episode_start"].copy(),
            "resource": (info & 0xFF).astype(np.int32), "finished": (info & INFO_FINISHED) != 0,
            "order": order.astype(np.int32), "first": first.astype(np.int32), "count": count.astype(np.int32),
            "start": recs["start"].copy(), "end": recs["end"].copy(),
            "from_loc": ((info >> 16) & 15).astype(np.int32), "to_loc": ((info >> 20) & 15).astype(np.int32),
            "records": recs, "dropped": int(dropped)}


def _as_dict(ops):
    return ops if isinstance(ops, dict) else records_dict(np.asarray(ops))


def _cfg(config, key):
    if config is None:
        config = nat.default_config()
    return int(config[key] if isinstance(config, dict) else getattr(config, key))


def gantt(ops, config=None):
    """The bars of a Gantt chart: {(env, episode_start, resource): dict of arrays} with the group's
    ops ordered by start and start_time / end_time = step * step_size beside the record's fields
    (end_time NaN for an unfinished op).  ops: ScheduleLog.pop()'s dict or an OP_DTYPE array;
    config: an fjsp_config or anything with step_size (None = the default config).  It groups any
    resource number, so PackagingLog.pop()'s dict (resources 4..7, one bar per tray run; an
    ungranted run has start = -1) goes through unchanged."""
    d = _as_dict(ops)
    step_size = float(_cfg(config, "step_size"))
    keys = ("order", "first", "count", "start", "end", "finished", "from_loc", "to_loc")
    n = len(d["env"])
    idx = np.lexsort((np.arange(n), d["start"], d["resource"], d["episode_start"], d["env"]))
    groups = {}
    for i in idx.tolist():
        groups.setdefault((int(d["env"][i]), int(d["episode_start"][i]), int(d["resource"][i])), []).append(i)
    out = {}
    for k, rows in groups.items():
        rows = np.asarray(rows)
        g = {f: d[f][rows] for f in keys}
        g["start_time"] = g["start"].astype(np.float64) * step_size
        g["end_time"] = np.where(g["finished"], g["end"].astype(np.float64) * step_size, np.nan)
        out[k] = g
    return out


def check(ops, config=None):
    """Raise ValueError unless, per (env, episode, resource), the ops do not overlap (each ends no
    later than the next starts; an unfinished op is the group's last) and every finished machine
    op lasts count * processing_time / step_size steps."""
    step_size = _cfg(config, "step_size")
    pts = {2: _cfg(config, "pt_small") // step_size, 3: _cfg(config, "pt_big") // step_size}
    for (env, es, res), g in gantt(ops, config).items():
        n = len(g["start"])
        for i in range(n):
            s, e, fin = int(g["start"][i]), int(g["end"][i]), bool(g["finished"][i])
            where = f"env {env} episode_start {es} resource {res} op {i}"
            if fin and e < s:
                raise ValueError(f"{where}: ends at {e} before its start {s}")
            if not fin and i != n - 1:
                raise ValueError(f"{where}: unfinished but not the last op of its episode")
            if i + 1 < n and fin and e > int(g["start"][i + 1]):
                raise ValueError(f"{where}: ends at {e}, after the next op's start {int(g['start'][i + 1])}")
            if fin and res in pts and e - s != int(g["count"][i]) * pts[res]:
                raise ValueError(f"{where}: lasts {e - s} steps, {int(g['count'][i])} products need "
                                 f"{int(g['count'][i]) * pts[res]}")


# ---- packaging runs ---------------------------------------------------------------------------
PACK_ROWS = 4                       # blue_1, blue_2, red, green = agents 4..7
STATIONS = ("packaging_blue_1", "packaging_blue_2", "packaging_red", "packaging_green")   # resource = 4 + index
RES_PACK_START, RES_AGV_TO_PACK = 1 << 1, 1 << 5
INFO_GRANTED = 1 << 9
LOC_PACKAGING = 5
PACK_CARRY_WORDS, PACK_RING = 10, 256


def pack_fields(word):
    """(runs, pending, completed) of a pack word (array or int): the tray runs at the station, the
    products queued + in flight, the products packaged this episode."""
    w = np.asarray(word).astype(np.int64) & 0xFFFFFFFF
    return w & 0xFF, (w >> 8) & 0xFFF, (w >> 20) & 0xFFF


def _pack_fresh():
    return {"ln": 0, "hprev": 0, "prev": [0] * PACK_ROWS, "fifo": [[] for _ in range(PACK_ROWS)]}


def packaging_reference(results, held, pack, term, trunc, state=None, step0=0, env_gid0=0):
    """The specification of fjsp_packaging_scan on the host, in plain Python ints.  results
    [T, 8, N], held [T, 3, N], pack [T, 4, N] (any integer dtype), term / trunc [T, N]; state = what
    an earlier call returned (None: fresh): per env the open episode's length, the previous row's
    AGV held word and pack words and per station the FIFO of [code, granted, start].  Returns
    (records, state): records an OP_DTYPE array in (t, env, station, FIFO position) order."""
    term = np.asarray(term)
    T, N = term.shape
    trunc = np.asarray(trunc).reshape(T, N)
    res = (np.asarray(results).astype(np.int64) & 0xFFFFFFFF).reshape(T, NA, N)
    hld = (np.asarray(held).astype(np.int64) & 0xFFFFFFFF).reshape(T, HELD_ROWS, N)
    pk = (np.asarray(pack).astype(np.int64) & 0xFFFFFFFF).reshape(T, PACK_ROWS, N)
    state = [_pack_fresh() for _ in range(N)] if state is None else \
        [{"ln": s["ln"], "hprev": s["hprev"], "prev": list(s["prev"]), "fifo": [[list(x) for x in f] for f in s["fifo"]]}
         for s in state]
    out = []
    for e in range(N):
        S = state[e]
        for t in range(T):
            end = bool(term[t, e]) or bool(trunc[t, e])
            ln, agv = S["ln"], int(res[t, 1, e])
            drop = agv & RES_AGV_DROP and agv & RES_AGV_TO_PACK
            pos = 0

            def write(s, run, fin):
                nonlocal pos
                code, granted, start = run
                info = (4 + s) | (INFO_FINISHED if fin else 0) | (INFO_GRANTED if granted else 0) | \
                    (LOC_PACKAGING << 16) | (LOC_PACKAGING << 20)
                out.append((t, e, pos, (env_gid0 + e, info, step0 + t - ln, code, start if granted else -1,
                                        ln if fin else -1, 0)))
                pos += 1
            for s in range(PACK_ROWS):
                now, prev, fifo = int(pk[t, s, e]), S["prev"][s], S["fifo"][s]
                rise = ((now >> 8) & 0xFFF) + (now >> 20) - ((prev >> 8) & 0xFFF) - (prev >> 20)
                if drop and rise > 0:
                    code = S["hprev"] & HELD_CODE_MASK
                    assert rise == (code >> 10) & 7, (t, e, s, rise, code)   # the device does not check this
                    fifo.append([code, 0, 0])
                if int(res[t, 4 + s, e]) & RES_PACK_START:
                    for run in fifo:
                        if not run[1]:
                            run[1], run[2] = 1, ln
                for _ in range(max(0, len(fifo) - (now & 0xFF))):
                    write(s, fifo.pop(0), True)
                if end:
                    while fifo:
                        write(s, fifo.pop(0), False)
                S["prev"][s] = 0 if end else now
            S["hprev"] = 0 if end else int(hld[t, 0, e])
            S["ln"] = 0 if end else ln + 1
    out.sort(key=lambda x: x[:3])
    recs = np.zeros(len(out), dtype=OP_DTYPE)
    for k, x in enumerate(out):
        recs[k] = x[3]
    return recs, state


def pack_records_dict(recs, dropped=0):
    """OP_DTYPE array of packaging records -> the dict PackagingLog.pop() returns: records_dict's
    fields plus station (0..3 = resource - 4) and granted."""
    d = records_dict(recs, dropped)
    d["station"] = d["resource"] - 4
    d["granted"] = (recs["info"].astype(np.int64) & INFO_GRANTED) != 0
    return d


def _as_pack_dict(pack_ops):
    return pack_ops if isinstance(pack_ops, dict) else pack_records_dict(np.asarray(pack_ops))


def check_packaging(pack_ops, config=None):
    """Raise ValueError unless every finished run lasts pt_packaging // step_size steps and, per
    (env, episode, station) in record order, start and end do not decrease (the granted runs'
    start, the finished runs' end) and no finished run follows an unfinished one."""
    d = _as_pack_dict(pack_ops)
    dur = _cfg(config, "pt_packaging") // _cfg(config, "step_size")
    last = {}   # group -> [last start, last end, an unfinished run seen]
    for i in range(len(d["env"])):
        key = (int(d["env"][i]), int(d["episode_start"][i]), int(d["resource"][i]))
        s, e, fin, granted = int(d["start"][i]), int(d["end"][i]), bool(d["finished"][i]), bool(d["granted"][i])
        where = f"env {key[0]} episode_start {key[1]} resource {key[2]} record {i}"
        g = last.setdefault(key, [-1, -1, False])
        if fin and not granted:
            raise ValueError(f"{where}: finished but never granted")
        if fin and e - s != dur:
            raise ValueError(f"{where}: lasts {e - s} steps, packaging takes {dur}")
        if fin and g[2]:
            raise ValueError(f"{where}: finished after an unfinished run of its station")
        if granted:
            if s < g[0]:
                raise ValueError(f"{where}: starts at {s}, before the previous run's start {g[0]}")
            g[0] = s
        if fin:
            if e < g[1]:
                raise ValueError(f"{where}: ends at {e}, before the previous run's end {g[1]}")
            g[1] = e
        else:
            g[2] = True


def arrivals(ops, pack_ops):
    """Per packaging record the step at which the AGV dropped that tray at packaging: the end of the
    finished AGV record with the same (env, episode_start, tray) and to_loc == 5, -1 where the log
    holds none.  start - arrival is the run's wait in the station's queue (a tray code is unique
    within an episode)."""
    a, p = _as_dict(ops), _as_pack_dict(pack_ops)
    drops = {}
    m = (a["resource"] == 1) & a["finished"] & (a["to_loc"] == LOC_PACKAGING)
    for i in np.flatnonzero(m).tolist():
        drops[(int(a["env"][i]), int(a["episode_start"][i]), int(a["records"]["tray"][i]))] = int(a["end"][i])
    return np.array([drops.get((int(p["env"][i]), int(p["episode_start"][i]), int(p["records"]["tray"][i])), -1)
                     for i in range(len(p["env"]))], dtype=np.int64)


def carry_words():
    return int(nat.lib().fjsp_schedule_carry_words())


def temp_bytes(T, N):
    n = ctypes.c_uint64()
    nat.check(nat.lib().fjsp_schedule_temp_bytes(int(T), int(N), ctypes.byref(n)))
    return int(n.value)


class ScheduleLog(SlabLog):
    """Device-resident operation log of num_envs envs: the carry of the open episodes (length, open
    ops), a record buffer of `capacity` fjsp_op_rec, the device-side record count and the running
    vector-step counter step0.  scan() appends without synchronising; pop() copies the records to
    the host (the only synchronisation) and empties the log."""
    REC_DTYPE = OP_DTYPE

    def __init__(self, num_envs, device, env_id_base=0, capacity=1 << 20):
        import torch
        super().__init__(num_envs, device, capacity, env_id_base)
        words = carry_words()
        assert words == CARRY_WORDS, (words, CARRY_WORDS)
        self.carry = torch.zeros(words, self.N, dtype=torch.int32, device=self.device)

    def _temp_bytes(self, T):
        return temp_bytes(T, self.N)

    def scan(self, results, held, term, trunc):
        """Compact the slab (contiguous device tensors: results int32 / uint32 [T, 8, N], held int32 /
        uint32 [T, 3, N], term / trunc u8 [T, N]) on the current stream; advances step0 by T."""
        import torch
        T, N = int(term.shape[0]), self.N
        self._launch(T, (("results", results, word_dtypes(), (T, NA, N), True),
                         ("held", held, word_dtypes(), (T, HELD_ROWS, N), True),
                         ("term", term, (torch.uint8,), (T, N), True),
                         ("trunc", trunc, (torch.uint8,), (T, N), True)),
                     lambda temp, nbytes, stream: nat.lib().fjsp_schedule_scan(
                         _ptr(results), _ptr(held), _ptr(term), _ptr(trunc), T, N, self.env_id_base, self.step0,
                         _ptr(self.carry), _ptr(self.recs), self.capacity, _ptr(self.count), temp, nbytes, stream))

    def pop(self):
        """Every record logged since the last pop as a dict of numpy arrays: env, episode_start,
        resource (1 AGV, 2 small machine, 3 big machine), finished, order, first, count, start,
        end, from_loc, to_loc, the raw `records` and dropped = the ops that did not fit the
        capacity.  Synchronises; empties the log (the carry of the open episodes is kept)."""
        return records_dict(*self.pop_records())


class PackagingLog(SlabLog):
    """Device-resident log of the packaging runs of num_envs envs (fjsp_packaging_scan): the carry
    of the open episodes, the per-station FIFO rings (4 KB per env), a record buffer of `capacity`
    fjsp_op_rec, the device-side record count and the running vector-step counter step0.  scan()
    appends without synchronising; pop() copies the records to the host and empties the log.
    reset() zeroes the carry only: an all-zero carry empties the env's FIFOs, so the rings need no
    clearing."""
    REC_DTYPE = OP_DTYPE

    def __init__(self, num_envs, device, env_id_base=0, capacity=1 << 20):
        import torch
        super().__init__(num_envs, device, capacity, env_id_base)
        words = int(nat.lib().fjsp_packaging_carry_words())
        assert words == PACK_CARRY_WORDS, (words, PACK_CARRY_WORDS)
        n = ctypes.c_uint64()
        nat.check(nat.lib().fjsp_packaging_ring_bytes(self.N, ctypes.byref(n)))
        assert n.value == PACK_ROWS * PACK_RING * 4 * self.N
        self.carry = torch.zeros(words, self.N, dtype=torch.int32, device=self.device)
        self.ring = torch.zeros(PACK_ROWS, PACK_RING, self.N, dtype=torch.int32, device=self.device)

    def _temp_bytes(self, T):
        n = ctypes.c_uint64()
        nat.check(nat.lib().fjsp_packaging_temp_bytes(int(T), self.N, ctypes.byref(n)))
        return int(n.value)

    def scan(self, results, held, pack, term, trunc):
        """Compact the slab (contiguous device tensors: results int32 / uint32 [T, 8, N], held
        [T, 3, N] and pack [T, 4, N] of the same dtypes, term / trunc u8 [T, N]) on the current
        stream; advances step0 by T."""
        import torch
        T, N = int(term.shape[0]), self.N
        self._launch(T, (("results", results, word_dtypes(), (T, NA, N), True),
                         ("held", held, word_dtypes(), (T, HELD_ROWS, N), True),
                         ("pack", pack, word_dtypes(), (T, PACK_ROWS, N), True),
                         ("term", term, (torch.uint8,), (T, N), True),
                         ("trunc", trunc, (torch.uint8,), (T, N), True)),
                     lambda temp, nbytes, stream: nat.lib().fjsp_packaging_scan(
                         _ptr(results), _ptr(held), _ptr(pack), _ptr(term), _ptr(trunc), T, N, self.env_id_base,
                         self.step0, _ptr(self.carry), _ptr(self.ring), _ptr(self.recs), self.capacity,
                         _ptr(self.count), temp, nbytes, stream))

    def pop(self):
        """Every packaging run logged since the last pop as a dict of numpy arrays: records_dict's
        fields (resource = 4 + station, from_loc = to_loc = 5) plus station (0..3) and granted."""
        return pack_records_dict(*self.pop_records())


__all__ = ["OP_DTYPE", "ScheduleLog", "schedule_reference", "gantt", "check", "records_dict", "tray_fields",
           "CARRY_WORDS", "carry_words", "temp_bytes", "PACK_ROWS", "pack_fields", "packaging_reference",
           "PackagingLog", "pack_records_dict", "check_packaging", "arrivals"]
