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


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class EpisodeLog:
    """Device-resident episode log of num_envs envs: the carry of the open episodes (per-agent
    sums, steps so far), a record buffer of `capacity` fjsp_episode_rec, the device-side episode
    count and the running vector-step counter step0.  scan() appends without synchronising;
    pop() copies the records to the host (the only synchronisation) and empties the log."""

    def __init__(self, num_envs, device, capacity=65536, env_id_base=0):
        import torch
        self.N = int(num_envs)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise nat.FjspNativeError("EpisodeLog needs a GPU (HIP); no CPU fallback exists")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity = int(capacity)
        self.env_id_base = int(env_id_base)
        self.acc = torch.zeros(NA, self.N, dtype=torch.float64, device=self.device)
        self.len = torch.zeros(self.N, dtype=torch.int32, device=self.device)
        self.recs = torch.zeros(max(self.capacity, 1) * REC_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.step0 = 0
        self._temp = None
        self._seq0 = 0   # episodes popped so far: seq keeps counting over the log's lifetime

    def _temp_for(self, T):
        import torch
        need = temp_bytes(T, self.N)
        if self._temp is None or self._temp.numel() < need:
            self._temp = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._temp

    def scan(self, rewards, term, trunc, orders_completed=None, packaged=None):
        """Account the [T, 8, N] slab (contiguous device tensors: rewards f64, term / trunc u8 [T, N],
        optional int32 infos slabs) on the current stream; advances step0 by T."""
        import torch
        T = int(rewards.shape[0])
        if tuple(rewards.shape) != (T, NA, self.N) or rewards.dtype != torch.float64:
            raise ValueError(f"rewards must be float64 [T, 8, {self.N}]")
        for name, x, dt in (("term", term, torch.uint8), ("trunc", trunc, torch.uint8),
                            ("orders_completed", orders_completed, torch.int32), ("packaged", packaged, torch.int32)):
            if x is not None and (tuple(x.shape) != (T, self.N) or x.dtype != dt):
                raise ValueError(f"{name} must be {dt} [T, {self.N}]")
        for x in (rewards, term, trunc, orders_completed, packaged):
            if x is not None and (not x.is_contiguous() or x.device != self.device):
                raise ValueError("EpisodeLog.scan takes contiguous tensors on the log's device")
        temp = self._temp_for(T)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(nat.lib().fjsp_episode_scan(
                _ptr(rewards), _ptr(term), _ptr(trunc), _ptr(orders_completed), _ptr(packaged), T, self.N,
                self.env_id_base, self.step0, _ptr(self.acc), _ptr(self.len), _ptr(self.recs), self.capacity,
                _ptr(self.count), _ptr(temp), temp.numel(), ctypes.c_void_p(stream)))
        self.step0 += T

    def pop_records(self):
        """(records, dropped): the records logged since the last pop as a REC_DTYPE array in seq
        order (the bytes the kernel wrote; seq counted over the log's lifetime) and the number that
        did not fit the capacity.  Synchronises; empties the log, keeps the carry."""
        count = int(self.count.item())
        n = min(count, self.capacity)
        recs = self.recs[:n * REC_DTYPE.itemsize].cpu().numpy().view(REC_DTYPE).copy()
        recs["seq"] += np.uint64(self._seq0)
        self._seq0 += count
        self.count.zero_()
        return recs, max(0, count - self.capacity)

    def pop(self):
        """Every record logged since the last pop, in seq order, as a dict of numpy arrays: env,
        length, end_step, seq, terminated, truncated, orders_completed, packaged, total, by_agent
        [8, n], and dropped = the episodes that did not fit the capacity.  Synchronises; empties
        the log (the carry of the open episodes is kept)."""
        return records_dict(*self.pop_records())

    def reset(self, env_mask=None):
        """Zero the carry of the selected envs (all by default): after a manual env.reset."""
        import torch
        if env_mask is None:
            self.acc.zero_()
            self.len.zero_()
            return
        m = torch.as_tensor(env_mask, device=self.device).bool()
        self.acc.masked_fill_(m[None, :], 0.0)
        self.len.masked_fill_(m, 0)

    def state(self):
        """The carry, step0 and the counts, for a checkpoint (records not yet popped are not part
        of it: pop() first)."""
        return {"acc": self.acc.cpu().numpy(), "len": self.len.cpu().numpy(), "step0": int(self.step0),
                "count": int(self.count.item()) + self._seq0}

    def load_state(self, st):
        import torch
        self.acc.copy_(torch.as_tensor(np.asarray(st["acc"], dtype=np.float64)))
        self.len.copy_(torch.as_tensor(np.asarray(st["len"], dtype=np.int32)))
        self.step0 = int(st["step0"])
        self._seq0 = int(st["count"])
        self.count.zero_()


__all__ = ["episodes_reference", "EpisodeLog", "REC_DTYPE", "records_dict", "temp_bytes"]
