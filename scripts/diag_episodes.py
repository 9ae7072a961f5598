#!/usr/bin/env python3
"""Episode-scan cost (diagnostic): fjsp_episode_scan's three launches together against
fjsp_gae_shared over the same 256 x 8 x 4 096 slab in one process (medians of hipEvent-bracketed
repetitions after a warm-up; the records are checked against episodes_reference on a sub-slab),
and learn()'s time per batch at 4 096 envs with episode tracking on and off.  Writes JSON
(default profiles/episodes/scan_ab.json)."""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
nat = importlib.import_module("multi-agent-rl-for-fjsp_amd._native")
EP = importlib.import_module("multi-agent-rl-for-fjsp_amd.episodes")
V = importlib.import_module("multi-agent-rl-for-fjsp_amd.vec_env")
A2C = importlib.import_module("multi-agent-rl-for-fjsp_amd.a2c_vec")


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
    v = torch.randn(T + 1, N, device=dev, generator=g)
    ret, adv = torch.empty_like(r), torch.empty_like(r)
    s = torch.cuda.current_stream(dev)
    episodes = int(done.sum().item())
    log = EP.EpisodeLog(N, dev, capacity=40 * episodes + 1024)   # every timed scan's records fit
    temp = log._temp_for(T)
    P = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    args = (P(r), P(term), P(trunc), None, None, T, N, 0, 0, P(log.acc), P(log.len), P(log.recs), log.capacity,
            P(log.count), P(temp), temp.numel(), ctypes.c_void_p(s.cuda_stream))

    def scan():   # the C entry directly, as gae_only below: one host call, three launches
        nat.check(nat.lib().fjsp_episode_scan(*args))

    d8 = (term | trunc).contiguous()

    def gae_only():
        nat.check(nat.lib().fjsp_gae_shared(ctypes.c_void_p(r.data_ptr()), ctypes.c_void_p(v.data_ptr()),
                                            ctypes.c_void_p(d8.data_ptr()), T, N, A, 0.99, 0.95,
                                            ctypes.c_void_p(ret.data_ptr()), ctypes.c_void_p(adv.data_ptr()),
                                            ctypes.c_void_p(s.cuda_stream)))
    res = {"T": T, "N": N, "episodes_in_slab": episodes}
    # alternate the two so that both see the same machine state
    res["episode_scan_3_launches"] = timed(scan, s)
    res["gae_shared"] = timed(gae_only, s)
    log.count.zero_()
    res["episode_scan_3_launches_again"] = timed(scan, s)
    res["gae_shared_again"] = timed(gae_only, s)
    res["scan_algo_bytes"] = T * A * N * 8 + 2 * T * N + episodes * 112
    res["gae_algo_bytes"] = T * A * N * 24 + (T + 1) * N * 4 + T * N
    # correctness at the timed size: the first 64 envs against the host specification
    log.reset()
    log.count.zero_()
    log.step0 = 0
    log._seq0 = 0
    log.scan(r, term, trunc)
    got, dropped = log.pop_records()
    sub = got[got["env_gid"] < 64]
    want, _, _ = EP.episodes_reference(r[:, :, :64].cpu().numpy(), term[:, :64].cpu().numpy(),
                                       trunc[:, :64].cpu().numpy())
    res["records_equal_reference_first_64_envs"] = bool(
        len(sub) == len(want) and all(sub[f].tobytes() == want[f].tobytes()
                                      for f in EP.REC_DTYPE.names if f != "seq"))
    res["records"] = int(len(got))
    res["dropped"] = int(dropped)
    return res


def learn_ab(N=4096, T=256, warm=4, reps=20):
    """One learner, one env, the same streams: batches (collect, [account_episodes], update,
    roll_over) alternately with and without the accounting call, each bracketed by device
    synchronisations.  Accounting does not change what is trained on, so both modes time the same
    work but for the scan."""
    L = A2C.VecMultiAgentA2C(V.FJSPVecEnv(N), batch_size=T, seed=3, track_episodes=True)
    L.reset(seeds=torch.arange(N), num_orders=25)
    times = {"tracking_off": [], "tracking_on": []}
    for i in range(warm + reps):
        name = "tracking_on" if i % 2 else "tracking_off"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.collect()
        if name == "tracking_on":
            L.account_episodes()
        L.update()
        L.roll_over()
        torch.cuda.synchronize()
        if i >= warm:
            times[name].append((time.perf_counter() - t0) * 1e3)
    out = {"N": N, "T": T}
    for name, ts in times.items():
        ts.sort()
        out[name] = {"ms_per_batch_median": ts[len(ts) // 2], "ms_min": ts[0], "ms_max": ts[-1], "batches": len(ts)}
    rec = L.episode_summary()
    out["episodes_logged"] = int(len(rec["total"]))
    out["dropped"] = int(rec["dropped"])
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "episodes", "scan_ab.json"))
    ap.add_argument("--no-learn", action="store_true")
    a = ap.parse_args()
    out = {"scan": {}}
    for T, N in ((256, 4096), (256, 32768), (37, 4096)):
        out["scan"][f"T{T}_N{N}"] = scan_ab(T, N)
        print(json.dumps({f"T{T}_N{N}": out["scan"][f"T{T}_N{N}"]}), flush=True)
    if not a.no_learn:
        out["learn"] = learn_ab()
        print(json.dumps({"learn": out["learn"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
