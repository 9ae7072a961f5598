#!/usr/bin/env python3
"""Packaging-scan cost (diagnostic).  (1) fjsp_packaging_scan's three launches against
fjsp_schedule_scan's over the same 256 x 4 096 and 256 x 32 768 slabs of a heuristic rollout
(2 orders), in one process, alternating (medians of 30 hipEvent-bracketed repetitions after a
warm-up; a repetition starts from the carry the previous one left, as a running log does, which
changes a few records at the slab's first rows and nothing of the walk; the records of a fresh
log are checked against packaging_reference on the first 64 envs).
(2) fjsp_step_sched against fjsp_step_held at 4 096 envs with fjsp_last_kernel_ms, alternating on
two handles in the same state (medians of 30 steps each).  Writes JSON (default
profiles/packaging/scan.json)."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
nat = importlib.import_module("multi-agent-rl-for-fjsp_amd._native")
V = importlib.import_module("multi-agent-rl-for-fjsp_amd.vec_env")
SC = importlib.import_module("multi-agent-rl-for-fjsp_amd.schedule")


def timed(call, stream, warm=5, reps=30):
    for _ in range(warm):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(stream)
        call()
        b.record(stream)
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return {"us_median": us[len(us) // 2], "us_min": us[0], "us_max": us[-1], "reps": reps}


def slabs(T, N):
    """T rows of a heuristic run (2 orders, auto-reset) through fjsp_actions + fjsp_step_sched."""
    env = V.FJSPVecEnv(N)
    env.reset(num_orders=2)
    b = V.Buffers(T, N, env.device, infos=True, held=True, pack=True)
    rows = [V.RowBuffers(b, t) for t in range(T)]
    act = torch.empty(8, N, dtype=torch.uint8, device=env.device)
    for t in range(T):
        env.actions("heuristic", step=t, out=act)
        env.step(act, buffers=rows[t], held=b.held[t], pack=b.pack[t])
    return b


def scan_ab(T, N):
    b = slabs(T, N)
    dev = b.term.device
    s = torch.cuda.current_stream(dev)
    slog = SC.ScheduleLog(N, dev, capacity=1)
    slog.scan(b.results, b.held, b.term, b.trunc)
    ops = int(slog.count.item())
    plog = SC.PackagingLog(N, dev, capacity=1)
    plog.scan(b.results, b.held, b.pack, b.term, b.trunc)
    runs = int(plog.count.item())
    slog = SC.ScheduleLog(N, dev, capacity=40 * ops + 1024)   # every timed scan's records fit
    plog = SC.PackagingLog(N, dev, capacity=40 * runs + 1024)
    stemp, ptemp = slog._temp_for(T), plog._temp_for(T)
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    sargs = (P(b.results), P(b.held), P(b.term), P(b.trunc), T, N, 0, 0, P(slog.carry), P(slog.recs), slog.capacity,
             P(slog.count), P(stemp), stemp.numel(), ctypes.c_void_p(s.cuda_stream))
    pargs = (P(b.results), P(b.held), P(b.pack), P(b.term), P(b.trunc), T, N, 0, 0, P(plog.carry), P(plog.ring),
             P(plog.recs), plog.capacity, P(plog.count), P(ptemp), ptemp.numel(), ctypes.c_void_p(s.cuda_stream))

    def sscan():   # the C entries directly: one host call, three launches each
        nat.check(nat.lib().fjsp_schedule_scan(*sargs))

    def pscan():
        nat.check(nat.lib().fjsp_packaging_scan(*pargs))
    res = {"T": T, "N": N, "ops_in_slab": ops, "runs_in_slab": runs}
    res["schedule_scan"] = timed(sscan, s)
    res["packaging_scan"] = timed(pscan, s)
    for log in (slog, plog):
        log.count.zero_()
        log.carry.zero_()
    res["schedule_scan_again"] = timed(sscan, s)
    res["packaging_scan_again"] = timed(pscan, s)
    res["packaging_over_schedule"] = min(res["packaging_scan"]["us_median"], res["packaging_scan_again"]["us_median"]) / \
        min(res["schedule_scan"]["us_median"], res["schedule_scan_again"]["us_median"])
    res["schedule_algo_bytes"] = 2 * T * N * 26 + ops * 32
    res["packaging_algo_bytes"] = T * N * (22 + 42) + runs * (32 + 12)   # count 22, write 42 bytes per row and env
    # correctness at the timed size: the first 64 envs against the host specification
    plog = SC.PackagingLog(N, dev, capacity=runs + 16)
    plog.scan(b.results, b.held, b.pack, b.term, b.trunc)
    got, dropped = plog.pop_records()
    c = lambda x: x[..., :64].cpu().numpy()  # noqa: E731
    want, _ = SC.packaging_reference(c(b.results), c(b.held), c(b.pack), c(b.term), c(b.trunc))
    res["records_equal_reference_first_64_envs"] = bool(got[got["env_gid"] < 64].tobytes() == want.tobytes())
    res["records"] = int(len(got))
    res["dropped"] = int(dropped)
    return res


def step_ab(N=4096, reps=30, warm=20):
    envs = [V.FJSPVecEnv(N), V.FJSPVecEnv(N)]
    for e in envs:
        e.reset(num_orders=30)
    bufs = [V.Buffers(1, N, envs[0].device, infos=True, next_obs=True) for _ in envs]
    held = [torch.zeros(3, N, dtype=torch.int32, device=envs[0].device) for _ in envs]
    pack = torch.zeros(4, N, dtype=torch.int32, device=envs[0].device)
    act = torch.empty(8, N, dtype=torch.uint8, device=envs[0].device)
    ms = {"fjsp_step_held": [], "fjsp_step_sched": []}
    for t in range(warm + reps):
        envs[0].actions("masked", step=t, out=act)
        envs[0].step(act, buffers=bufs[0], held=held[0])
        a = envs[0].last_kernel_ms()
        envs[1].step(act, buffers=bufs[1], held=held[1], pack=pack)
        h = envs[1].last_kernel_ms()
        if t >= warm:
            ms["fjsp_step_held"].append(a * 1e3)
            ms["fjsp_step_sched"].append(h * 1e3)
    same = envs[0].snapshot().cpu().numpy().tobytes() == envs[1].snapshot().cpu().numpy().tobytes()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    return {"N": N, "reps": reps, "kernel": envs[0].last_kernel(), "states_equal": bool(same),
            "fjsp_step_held_us_median": med(ms["fjsp_step_held"]), "fjsp_step_sched_us_median": med(ms["fjsp_step_sched"]),
            "fjsp_step_held_us_min": min(ms["fjsp_step_held"]), "fjsp_step_sched_us_min": min(ms["fjsp_step_sched"])}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "packaging", "scan.json"))
    a = ap.parse_args()
    out = {"scan": {}}
    for T, N in ((256, 4096), (256, 32768)):
        out["scan"][f"T{T}_N{N}"] = scan_ab(T, N)
        print(json.dumps({f"T{T}_N{N}": out["scan"][f"T{T}_N{N}"]}), flush=True)
    out["step"] = step_ab()
    print(json.dumps({"step": out["step"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
