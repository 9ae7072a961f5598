#!/usr/bin/env python3
"""What track_kpis costs the A2C collect (profiles/train_kpis): collect time per 256 x N batch with
the switch off or on, and with it on account_kpis()'s scan time (HIP events).  Default launch path
of the learner (two env groups on two streams, eager).  Prints one JSON line.

One learner per process, and the runs to compare alternated process by process: a second learner
in the same process brings two more streams, and with the runtime's few hardware queues both of
its env groups can land on one queue, which serialises its collect (profiles/train_kpis/README.md).
Switch off against another build (e.g. the parent commit's library): --modes off once per
library, alternating the two (FJSP_LIB selects the library); compare the medians and their spreads.

usage: [FJSP_LIB=...] python scripts/measure_train_kpis.py [--n 4096] [--reps 12] [--modes off|on]"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
A = importlib.import_module("multi-agent-rl-for-fjsp_amd.a2c_vec")
V = importlib.import_module("multi-agent-rl-for-fjsp_amd.vec_env")
nat = importlib.import_module("multi-agent-rl-for-fjsp_amd._native")


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "all": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--modes", default="on", help="off | on (off,on: both in one process, see above)")
    a = ap.parse_args()
    modes = a.modes.split(",")
    learners = {}
    for m in modes:
        kw = {"track_kpis": True} if m == "on" else {}
        L = A.VecMultiAgentA2C(V.FJSPVecEnv(a.n), batch_size=a.T, seed=3, **kw)
        L.reset(seeds=torch.arange(a.n), num_orders=25)
        for _ in range(3):
            L.collect()
            if m == "on":
                L.account_kpis()
            L.roll_over()
        learners[m] = L
    torch.cuda.synchronize()
    ms = {m: [] for m in modes}
    scan = []
    for _ in range(a.reps):
        for m in modes:
            L = learners[m]
            t0 = time.perf_counter()
            L.collect()
            torch.cuda.synchronize()
            ms[m].append((time.perf_counter() - t0) * 1e3)
            if m == "on":
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                L.account_kpis()
                e1.record()
                torch.cuda.synchronize()
                scan.append(e0.elapsed_time(e1))
            L.roll_over()
    res = {"lib": os.path.basename(nat.LIB_PATH), "envs": a.n, "batch": a.T, "reps": a.reps,
           "kernel": learners[modes[0]].env.last_kernel(), "collect_ms": {m: stats(v) for m, v in ms.items()}}
    if scan:
        L = learners["on"]
        L.kpi_log.pop()
        slab = sum(L._bufs[k].numel() * L._bufs[k].element_size()
                   for k in ("results", "term", "trunc", "obs_i8", "orders_completed", "packaged", "sim_time"))
        res["kpi_scan_ms"] = stats(scan)
        res["kpi_scan_slab_bytes"] = slab
        res["kpi_scan_gb_per_s"] = slab / (res["kpi_scan_ms"]["median"] * 1e-3) / 1e9
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
