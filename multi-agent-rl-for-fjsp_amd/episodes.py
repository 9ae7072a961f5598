"""Episode accounting: returns, lengths and end steps of every finished episode of a rollout.

MultiAgentA2C.learn (a2c.py:254-388) keeps, per episode, each agent's summed rewards
(:311-313), their total (:348 -> overall_rewards), the step count it ended at (:350 ->
episode_end_timesteps) and the printed summary (:373-376).  ``episodes_reference`` restates that
arithmetic per env in plain Python floats (the specification); ``EpisodeLog`` is the same scan on
the device (fjsp_episode_scan, csrc/fjsp_episode.hip) over any [T, 8, N] slab, appending records
to a device-resident log with no host synchronisation until ``pop()``.
"""
import ctypes

import numpy as np

from . import _native as nat
from .slablog import EpisodeSlabLog, _ptr

NA = 8
FLAG_TERMINATED, FLAG_TRUNCATED = 1, 2

# include/fjsp.h fjsp_episode_rec (112 bytes)
REC_DTYPE = np.dtype([("env_gid", "<u4"), ("length", "<i4"), ("end_step", "<i8"), ("seq", "<u8"),
                      ("flags", "<i4"), ("orders_completed", "<i4"), ("packaged", "<i4"), ("reserved", "<i4"),
                      ("total", "<f8"), ("by_agent", "<f8", (NA,))])
assert REC_DTYPE.itemsize == 112


def episodes_reference(rewards, term, trunc, orders_completed=None, packaged=None, acc=None, length=None,
                       step0=0, env_gid0=0, seq0=0):
    """The specification of fjsp_episode_scan on the host: rewards [T, 8, N] (fp64), term / trunc
    [T, N], optional infos slabs [T, N]; acc [8, N] / length [N] = the carry of the open episodes
    (None: fresh).  Returns (records, acc, length): records a REC_DTYPE array in (t, e) order,
    numbered from seq0, and the carry after the slab.

    Per env this is a2c.py:311-313 (``episode_rewards[agent] += reward`` per step, Python
    floats) and :348 (``sum(episode_rewards.values())``: left to right from int 0)."""
    rewards = np.asarray(rewards, dtype=np.float64)
    T, A, N = rewards.shape
    assert A == NA
    term = np.asarray(term).reshape(T, N)
    trunc = np.asarray(trunc).reshape(T, N)
    oc = None if orders_completed is None else np.asarray(orders_completed).reshape(T, N)
    pk = None if packaged is None else np.asarray(packaged).reshape(T, N)
    ep = [[0.0] * NA for _ in range(N)] if acc is None else [[float(acc[a][e]) for a in range(NA)] for e in range(N)]
    ln = [0] * N if length is None else [int(x) for x in length]
    out = []
    for t in range(T):
        row = rewards[t].tolist()
        te, tr = term[t].tolist(), trunc[t].tolist()
        for e in range(N):
            er = ep[e]
            for a in range(NA):
                er[a] += row[a][e]                     # a2c.py:312-313
            ln[e] += 1
            if te[e] or tr[e]:
                total = sum(er)                        # a2c.py:348
                out.append((env_gid0 + e, ln[e], step0 + t + 1, seq0 + len(out),
                            (FLAG_TERMINATED if te[e] else 0) | (FLAG_TRUNCATED if tr[e] else 0),
                            -1 if oc is None else int(oc[t, e]), -1 if pk is None else int(pk[t, e]), 0,
                            float(total), tuple(er)))
                ep[e] = [0.0] * NA                     # a2c.py:381 defaultdict(float)
                ln[e] = 0
    recs = np.array(out, dtype=REC_DTYPE) if out else np.zeros(0, dtype=REC_DTYPE)
    acc_out = np.array(ep, dtype=np.float64).T.copy() if N else np.zeros((NA, 0))
    return recs, acc_out, np.array(ln, dtype=np.int32)


def records_dict(recs, dropped=0):
    """REC_DTYPE array -> the dict of arrays EpisodeLog.pop() returns."""
    return {"env": recs["env_gid"].copy(), "length": recs["length"].copy(), "end_step": recs["end_step"].copy(),
            "seq": recs["seq"].copy(), "terminated": (recs["flags"] & FLAG_TERMINATED) != 0,
            "truncated": (recs["flags"] & FLAG_TRUNCATED) != 0, "orders_completed": recs["orders_completed"].copy(),
            "packaged": recs["packaged"].copy(), "total": recs["total"].copy(),
            "by_agent": np.ascontiguousarray(recs["by_agent"].T), "dropped": int(dropped)}


def temp_bytes(T, N):
    n = ctypes.c_uint64()
    nat.check(nat.lib().fjsp_episode_temp_bytes(int(T), int(N), ctypes.byref(n)))
    return int(n.value)


class EpisodeLog(EpisodeSlabLog):
    """Device-resident episode log of num_envs envs: the carry of the open episodes (per-agent
    sums, steps so far), a record buffer of `capacity` fjsp_episode_rec, the device-side episode
    count and the running vector-step counter step0.  scan() appends without synchronising;
    pop() copies the records to the host (the only synchronisation) and empties the log."""
    REC_DTYPE = REC_DTYPE
    CARRY = ("acc", "len")

    def __init__(self, num_envs, device, capacity=65536, env_id_base=0):
        import torch
        super().__init__(num_envs, device, capacity, env_id_base)
        self.acc = torch.zeros(NA, self.N, dtype=torch.float64, device=self.device)
        self.len = torch.zeros(self.N, dtype=torch.int32, device=self.device)

    def _temp_bytes(self, T):
        return temp_bytes(T, self.N)

    def scan(self, rewards, term, trunc, orders_completed=None, packaged=None):
        """Account the [T, 8, N] slab (contiguous device tensors: rewards f64, term / trunc u8 [T, N],
        optional int32 infos slabs) on the current stream; advances step0 by T."""
        import torch
        T, N = int(rewards.shape[0]), self.N
        self._launch(T, (("rewards", rewards, (torch.float64,), (T, NA, N), True),
                         ("term", term, (torch.uint8,), (T, N), True),
                         ("trunc", trunc, (torch.uint8,), (T, N), True),
                         ("orders_completed", orders_completed, (torch.int32,), (T, N), False),
                         ("packaged", packaged, (torch.int32,), (T, N), False)),
                     lambda temp, nbytes, stream: nat.lib().fjsp_episode_scan(
                         _ptr(rewards), _ptr(term), _ptr(trunc), _ptr(orders_completed), _ptr(packaged), T, N,
                         self.env_id_base, self.step0, _ptr(self.acc), _ptr(self.len), _ptr(self.recs), self.capacity,
                         _ptr(self.count), temp, nbytes, stream))

    def pop(self):
        """Every record logged since the last pop, in seq order, as a dict of numpy arrays: env,
        length, end_step, seq, terminated, truncated, orders_completed, packaged, total, by_agent
        [8, n], and dropped = the episodes that did not fit the capacity.  Synchronises; empties
        the log (the carry of the open episodes is kept)."""
        return records_dict(*self.pop_records())


__all__ = ["episodes_reference", "EpisodeLog", "REC_DTYPE", "records_dict", "temp_bytes"]
