"""What the device-resident slab logs share (episodes.EpisodeLog, kpis.KpiLog, schedule.ScheduleLog,
schedule.PackagingLog), and the set of them an evaluation run scans its chunks into.

Each log reduces [T, ..., N] rollout slabs to records on the device (csrc/fjsp_episode.hip): it
owns a record buffer of `capacity` records, the device-side record count, the carry of the open
episodes and the running vector-step counter step0.  scan() appends without synchronising;
pop() copies the records to the host (the only synchronisation) and empties the log.
"""
import ctypes

import numpy as np

from . import _native as nat


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def check_slabs(owner, table, device):
    """The argument check of `owner`.scan.  table: rows (name, tensor, dtypes, shape, required); a
    tensor that is None passes unless required.  Needs no GPU."""
    for name, x, dts, shape, required in table:
        if x is None:
            if required:
                raise ValueError(f"{name} is required")
            continue
        if tuple(x.shape) != tuple(shape) or x.dtype not in dts:
            raise ValueError(f"{name} must be {dts[0]} {list(shape)}")
        if not x.is_contiguous() or x.device != device:
            raise ValueError(f"{owner}.scan takes contiguous tensors on the log's device")


def word_dtypes():
    """The dtypes a slab of 32-bit words may have."""
    import torch
    return (torch.int32, getattr(torch, "uint32", torch.int32))


class SlabLog:
    """The common part of the four logs.  A subclass sets REC_DTYPE (the record's numpy dtype),
    CARRY (the names of its carry tensors, [..., N] each), SEQ (its records have a `seq` counted
    over the log's lifetime) and _temp_bytes(T); it allocates its carry after calling __init__."""
    REC_DTYPE = None
    CARRY = ("carry",)
    SEQ = False

    def __init__(self, num_envs, device, capacity, env_id_base):
        import torch
        self.N = int(num_envs)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise nat.FjspNativeError(f"{type(self).__name__} needs a GPU (HIP); no CPU fallback exists")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.capacity = int(capacity)
        self.env_id_base = int(env_id_base)
        self.recs = torch.zeros(max(self.capacity, 1) * self.REC_DTYPE.itemsize, dtype=torch.uint8, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.step0 = 0
        self._temp = None
        self._seq0 = 0   # SEQ: records popped so far

    def _temp_for(self, T):
        import torch
        need = self._temp_bytes(T)
        if self._temp is None or self._temp.numel() < need:
            self._temp = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._temp

    def _launch(self, T, table, call):
        """Check the slabs, then call(temp, temp_bytes, stream) -> the entry's status on the current
        stream; advances step0 by T.  `call` reads the log's buffers when it runs."""
        import torch
        check_slabs(type(self).__name__, table, self.device)
        temp = self._temp_for(T)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(call(_ptr(temp), temp.numel(), ctypes.c_void_p(stream)))
        self.step0 += T

    def pop_records(self):
        """(records, dropped): the records logged since the last pop as a REC_DTYPE array in the
        order they were numbered (the bytes the kernel wrote; a `seq` counted over the log's
        lifetime) and the number that did not fit the capacity.  Synchronises; empties the log,
        keeps the carry."""
        count = int(self.count.item())
        n = min(count, self.capacity)
        recs = self.recs[:n * self.REC_DTYPE.itemsize].cpu().numpy().view(self.REC_DTYPE).copy()
        if self.SEQ:
            recs["seq"] += np.uint64(self._seq0)
            self._seq0 += count
        self.count.zero_()
        return recs, max(0, count - self.capacity)

    def reset(self, env_mask=None):
        """Zero the carry of the selected envs (all by default): after a manual env.reset."""
        import torch
        m = None if env_mask is None else torch.as_tensor(env_mask, device=self.device).bool()
        for name in self.CARRY:
            t = getattr(self, name)
            if m is None:
                t.zero_()
            else:
                t.masked_fill_(m if t.dim() == 1 else m[None, :], 0)


class EpisodeSlabLog(SlabLog):
    """A log with one record per finished episode: `seq` keeps counting over the log's lifetime, and
    the carry can be checkpointed."""
    SEQ = True

    def state(self):
        """The carry, step0 and the counts, for a checkpoint (records not yet popped are not part
        of it: pop() first)."""
        st = {name: getattr(self, name).cpu().numpy() for name in self.CARRY}
        st.update(step0=int(self.step0), count=int(self.count.item()) + self._seq0)
        return st

    def load_state(self, st):
        import torch
        for name in self.CARRY:
            t = getattr(self, name)
            t.copy_(torch.as_tensor(np.asarray(st[name])).to(t.dtype))
        self.step0 = int(st["step0"])
        self._seq0 = int(st["count"])
        self.count.zero_()


def capacities(num_envs, steps):
    """Record capacities of an evaluation run of `steps` vector steps.  What does not fit is counted
    in a result's `dropped`, never written."""
    N, steps = int(num_envs), int(steps)
    return {
        # one episode per 16 steps and env (the shortest heuristic episodes take ~30)
        "episodes": max(65536, N * (steps // 16 + 1)),
        # an op takes at least one step per resource, an AGV op two (pickup, drop): 3 per 2 steps bounds it
        "ops": max(65536, N * (3 * steps // 2 + 3)),
        # a packaging run needs an AGV carry (two steps) before it
        "pack_ops": max(65536, N * (steps // 2 + 1)),
    }


class LogSet:
    """The logs of one evaluation run over env: an EpisodeLog, and on request a KpiLog, a ScheduleLog
    and a PackagingLog, all scanned with the same rows."""
    SLABS = ("rewards", "term", "trunc", "orders_completed", "packaged", "results", "obs_i8", "sim_time", "held", "pack")

    def __init__(self, env, steps, kpis=True, schedule=False, packaging=False, device=None):
        from .episodes import EpisodeLog
        from .kpis import KpiLog
        from .schedule import PackagingLog, ScheduleLog
        cap = capacities(env.num_envs, steps)
        make = lambda cls, c: cls(env.num_envs, env.device if device is None else device,  # noqa: E731
                                  env_id_base=env.env_id_base, capacity=c)
        self.episodes = make(EpisodeLog, cap["episodes"])
        self.kpis = make(KpiLog, cap["episodes"]) if kpis else None
        self.ops = make(ScheduleLog, cap["ops"]) if schedule else None
        self.pack_ops = make(PackagingLog, cap["pack_ops"]) if packaging else None

    def scan(self, slabs, k):
        """Scan rows [:k] of the slabs (a mapping name -> [T, ..., N] tensor; SLABS' names are read,
        and those the set's logs do not take may be missing or None) into every log."""
        s = {n: slabs[n][:k] for n in self.SLABS if slabs.get(n) is not None}
        self.episodes.scan(s["rewards"], s["term"], s["trunc"], s["orders_completed"], s["packaged"])
        if self.kpis is not None:
            self.kpis.scan(s["results"], s["term"], s["trunc"], s["obs_i8"], s["orders_completed"], s["packaged"],
                           s["sim_time"])
        if self.ops is not None:
            self.ops.scan(s["results"], s["held"], s["term"], s["trunc"])
        if self.pack_ops is not None:
            self.pack_ops.scan(s["results"], s["held"], s["pack"], s["term"], s["trunc"])

    def pop(self):
        """{"episodes", "kpis", "ops", "pack_ops"}: every log's pop(), the logs that were asked for."""
        return {name: log.pop() for name in ("episodes", "kpis", "ops", "pack_ops")
                for log in (getattr(self, name),) if log is not None}


__all__ = ["SlabLog", "EpisodeSlabLog", "LogSet", "capacities", "check_slabs"]
