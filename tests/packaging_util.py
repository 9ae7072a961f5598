"""Shared inputs of the packaging tests: tests/golden/packaging.npz (the reference's pack words and
tray-run lists, gen_packaging_golden.py) beside the recorded traces."""
import functools

import numpy as np

from tests import episodes_util as U
from tests import schedule_util as SU

schedule = __import__("importlib").import_module("multi-agent-rl-for-fjsp_amd.schedule")

RUN_COLS = ("station", "finished", "granted", "episode_start", "tray", "start", "end", "drop")
TRACE_KEYS = [f"{p}_s{s}" for p, s in SU.RUNS]
SCRIPTED_KEYS = ["lazy12_s0", "lazy12_s1", "eager_long_s0", "eager_long_s1", "lazy7_long_s0", "lazy7_long_s1",
                 "eager_cap5_s0"]
KEYS = TRACE_KEYS + SCRIPTED_KEYS


@functools.lru_cache(maxsize=None)
def run(key):
    """One recorded run as a one-env slab: actions u8 [T, 8], results u32 [T, 8, 1], held u32
    [T, 3, 1], pack u32 [T, 4, 1], term / trunc u8 [T, 1], packaged i32 [T], runs i64 [n, 8] (RUN_COLS),
    orders u8 [episodes, num_orders, 3], cfg i32 [4] (pt_packaging, max_episode_steps, capacity,
    num_orders)."""
    pk = U._npz("packaging")
    src = pk if key in SCRIPTED_KEYS else U._npz("traces")
    out = {"actions": src[f"{key}_actions"].astype(np.uint8),
           "results": np.ascontiguousarray(src[f"{key}_results"].astype(np.uint32)[:, :, None]),
           "term": src[f"{key}_term"].astype(np.uint8)[:, None], "trunc": src[f"{key}_trunc"].astype(np.uint8)[:, None],
           "held": np.ascontiguousarray(pk[f"{key}_held"].astype(np.uint32)[:, :, None]),
           "pack": np.ascontiguousarray(pk[f"{key}_pack"].astype(np.uint32)[:, :, None]),
           "packaged": pk[f"{key}_packaged"].astype(np.int32), "runs": pk[f"{key}_runs"].astype(np.int64),
           "orders": pk[f"{key}_orders"], "cfg": pk[f"{key}_cfg"].astype(np.int32)}
    for v in out.values():
        v.setflags(write=False)
    return out


def fixture_records(runs, env_gid=0):
    """The fixture's run list as the OP_DTYPE records the scan writes for it."""
    c = {k: runs[:, i] for i, k in enumerate(RUN_COLS)}
    recs = np.zeros(len(runs), dtype=schedule.OP_DTYPE)
    recs["env_gid"] = env_gid
    recs["info"] = (4 + c["station"]) | (c["finished"] << 8) | (c["granted"] << 9) | (5 << 16) | (5 << 20)
    recs["episode_start"] = c["episode_start"]
    recs["tray"] = c["tray"]
    recs["start"] = c["start"]
    recs["end"] = c["end"]
    return recs


def contents(recs, pt_steps):
    """What a record array holds of the cases the scan is for: batches of >= 2 runs, pairs of
    overlapping batches at one station, granted-unfinished and ungranted runs, records at blue_2."""
    info = recs["info"].astype(np.int64)
    granted, fin = (info & 0x200) != 0, (info & 0x100) != 0
    batches = {}
    for i in np.flatnonzero(granted).tolist():
        k = (int(recs["env_gid"][i]), int(info[i] & 0xFF), int(recs["episode_start"][i]), int(recs["start"][i]))
        batches[k] = batches.get(k, 0) + 1
    keys = sorted(batches)
    return {"multi": sum(v >= 2 for v in batches.values()),
            "overlap": sum(a[:3] == b[:3] and b[3] - a[3] < pt_steps for a, b in zip(keys, keys[1:])),
            "granted_unfinished": int((granted & ~fin).sum()), "ungranted": int((~granted).sum()),
            "blue_2": int(((info & 0xFF) == 5).sum())}
