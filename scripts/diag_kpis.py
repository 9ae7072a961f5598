#!/usr/bin/env python3
"""KPI-scan cost (diagnostic): fjsp_kpi_scan's three launches against fjsp_episode_scan's over the
same 256 x 4 096 and 256 x 32 768 slabs in one process, alternating (medians of 30
hipEvent-bracketed repetitions after a warm-up, done density ~1/201; the KPI records are checked
against kpi_reference on the first 64 envs); with --subsets also fjsp_kpi_scan with only some of its
optional slabs given, which shows what each slab's loads cost.  Writes JSON (default
profiles/kpi/scan.json)."""
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
EP = importlib.import_module("multi-agent-rl-for-fjsp_amd.episodes")
KP = importlib.import_module("multi-agent-rl-for-fjsp_amd.kpis")


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


def scan_ab(T, N, A=8, density=1.0 / 201):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    r = ((torch.randn(T, A, N, device=dev, generator=g, dtype=torch.float64) * 24).round() / 8).contiguous()
    done = torch.rand(T, N, device=dev, generator=g) < density
    kind = torch.rand(T, N, device=dev, generator=g) < 0.5
    term = (done & kind).to(torch.uint8)
    trunc = (done & ~kind).to(torch.uint8)
    ri = lambda hi, *s, dt=torch.int32: torch.randint(0, hi, s, device=dev, generator=g).to(dt)  # noqa: E731
    results = (ri(256, T, A, N) | (ri(64, T, A, N) << 16)).contiguous()
    obs = ri(8, T, 12, N, dt=torch.int8)
    oc = torch.cumsum(ri(2, T, N) * (ri(40, T, N) == 0), 0).to(torch.int32).contiguous()
    pk = torch.cumsum(ri(2, T, N) * (ri(8, T, N) == 0), 0).to(torch.int32).contiguous()
    st = (torch.arange(1, T + 1, device=dev, dtype=torch.float64)[:, None] * 10.0).expand(T, N).contiguous()
    s = torch.cuda.current_stream(dev)
    episodes = int(done.sum().item())
    elog = EP.EpisodeLog(N, dev, capacity=40 * episodes + 1024)   # every timed scan's records fit
    klog = KP.KpiLog(N, dev, capacity=40 * episodes + 1024)
    temp = elog._temp_for(T)
    ktemp = klog._temp_for(T)
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    eargs = (P(r), P(term), P(trunc), P(oc), P(pk), T, N, 0, 0, P(elog.acc), P(elog.len), P(elog.recs), elog.capacity,
             P(elog.count), P(temp), temp.numel(), ctypes.c_void_p(s.cuda_stream))
    kargs = (P(results), P(term), P(trunc), P(obs), P(oc), P(pk), P(st), T, N, 0, 0, P(klog.carry), P(klog.recs),
             klog.capacity, P(klog.count), P(ktemp), ktemp.numel(), ctypes.c_void_p(s.cuda_stream))

    def escan():   # the C entries directly: one host call, three launches each
        nat.check(nat.lib().fjsp_episode_scan(*eargs))

    def kscan():
        nat.check(nat.lib().fjsp_kpi_scan(*kargs))
    res = {"T": T, "N": N, "episodes_in_slab": episodes}
    # alternate the two so that both see the same machine state
    res["episode_scan"] = timed(escan, s)
    res["kpi_scan"] = timed(kscan, s)
    elog.count.zero_()
    klog.count.zero_()
    res["episode_scan_again"] = timed(escan, s)
    res["kpi_scan_again"] = timed(kscan, s)
    res["kpi_over_episode"] = min(res["kpi_scan"]["us_median"], res["kpi_scan_again"]["us_median"]) / \
        min(res["episode_scan"]["us_median"], res["episode_scan_again"]["us_median"])
    res["episode_algo_bytes"] = T * N * (A * 8 + 2) + episodes * (112 + 8)
    res["kpi_algo_bytes"] = T * N * (A * 4 + 12 + 8 + 2) + episodes * (432 + 12)
    # correctness at the timed size: the first 64 envs against the host specification
    klog.reset()
    klog.count.zero_()
    klog.step0 = 0
    klog._seq0 = 0
    klog.scan(results, term, trunc, obs, oc, pk, st)
    got, dropped = klog.pop_records()
    sub = got[got["env_gid"] < 64]
    c = lambda x: x[..., :64].cpu().numpy()  # noqa: E731
    want, _ = KP.kpi_reference(c(results), c(term), c(trunc), c(obs), c(oc), c(pk), c(st))
    res["records_equal_reference_first_64_envs"] = bool(
        len(sub) == len(want) and all(sub[f].tobytes() == want[f].tobytes()
                                      for f in KP.KPI_DTYPE.names if f != "seq"))
    res["records"] = int(len(got))
    res["dropped"] = int(dropped)
    return res


def subsets(T, N):
    """us_median of fjsp_kpi_scan with subsets of the optional slabs given, and with no episode end."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    term = (torch.rand(T, N, device=dev, generator=g) < 1.0 / 201).to(torch.uint8)
    trunc = torch.zeros_like(term)
    ri = lambda hi, *s, dt=torch.int32: torch.randint(0, hi, s, device=dev, generator=g).to(dt)  # noqa: E731
    results = (ri(256, T, 8, N) | (ri(64, T, 8, N) << 16)).contiguous()
    obs = ri(8, T, 12, N, dt=torch.int8)
    oc = torch.cumsum(ri(2, T, N) * (ri(40, T, N) == 0), 0).to(torch.int32).contiguous()
    pk = torch.cumsum(ri(2, T, N) * (ri(8, T, N) == 0), 0).to(torch.int32).contiguous()
    st = (torch.arange(1, T + 1, device=dev, dtype=torch.float64)[:, None] * 10.0).expand(T, N).contiguous()
    s = torch.cuda.current_stream(dev)
    klog = KP.KpiLog(N, dev, capacity=80 * int(term.sum().item()) + 1024)
    temp = klog._temp_for(T)
    P = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731

    def time_of(r_, te, o_, c_, p_, t_):
        args = (P(r_), P(te), P(trunc), P(o_), P(c_), P(p_), P(t_), T, N, 0, 0, P(klog.carry), P(klog.recs),
                klog.capacity, P(klog.count), P(temp), temp.numel(), ctypes.c_void_p(s.cuda_stream))
        klog.count.zero_()
        return round(timed(lambda: nat.check(nat.lib().fjsp_kpi_scan(*args)), s)["us_median"], 1)
    sets = {"all": (results, obs, oc, pk, st), "none": (None,) * 5, "results": (results, None, None, None, None),
            "obs_i8": (None, obs, None, None, None), "infos": (None, None, oc, pk, None),
            "sim_time": (None, None, None, None, st), "results+obs_i8": (results, obs, None, None, None)}
    out = {name: time_of(r_, term, o_, c_, p_, t_) for name, (r_, o_, c_, p_, t_) in sets.items()}
    out["all_no_episode_ends"] = time_of(results, torch.zeros_like(term), obs, oc, pk, st)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "kpi", "scan.json"))
    ap.add_argument("--subsets", action="store_true")
    a = ap.parse_args()
    out = {"scan": {}}
    for T, N in ((256, 4096), (256, 32768)):
        out["scan"][f"T{T}_N{N}"] = scan_ab(T, N)
        print(json.dumps({f"T{T}_N{N}": out["scan"][f"T{T}_N{N}"]}), flush=True)
    if a.subsets:
        out["subsets_us_median"] = {f"T{T}_N{N}": subsets(T, N) for T, N in ((256, 4096), (256, 32768))}
        print(json.dumps({"subsets_us_median": out["subsets_us_median"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
