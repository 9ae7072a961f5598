#!/usr/bin/env python3
"""Rollout search cost (diagnostic).  4 096 lanes = 128 five-order books x 32 replicas, K = 201.
(1) one pass-0 launch of k_search_rollout (fjsp_search_rollout, eps8 = 38) from the reset state;
(2) the same 201 steps as fjsp_actions(heuristic) + fjsp_step per step (402 launches, the step's full
outputs written every step); (3) the same with fjsp_actions_eps in place of fjsp_actions.  Each is
bracketed by hipEvents on the stream, from the restored reset state, alternating, medians of `reps`
repetitions after a warm-up.  (4) the wall time of a whole FJSPVecEnv.search at stride 8, with its
passes and what it found.  Writes JSON (default profiles/search/search.json)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
V = importlib.import_module("multi-agent-rl-for-fjsp_amd.vec_env")
O = importlib.import_module("multi-agent-rl-for-fjsp_amd.orders")


def books_of(n, orders, seed=1):
    rng = np.random.RandomState(seed)
    return [[(int(rng.randint(1, 10)), int(rng.randint(1, 4)), int(rng.randint(1, 4))) for _ in range(orders)]
            for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--books", type=int, default=128)
    ap.add_argument("--width", type=int, default=32)
    ap.add_argument("--orders", type=int, default=5)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "search", "search.json"))
    a = ap.parse_args()
    books, W = books_of(a.books, a.orders), a.width
    N, K = a.books * W, 201
    env = V.FJSPVecEnv(N)
    words, counts = O.encode([b for b in books for _ in range(W)])
    env.reset_orders(words, counts)
    start = env.snapshot().clone()
    stream = torch.cuda.current_stream(env.device)
    trace = torch.zeros(K, 8, N, dtype=torch.uint8, device=env.device)
    end = V.SearchEnd(N, env.device)
    buf = V.Buffers(1, N, env.device, infos=True, next_obs=True)
    act = torch.empty(8, N, dtype=torch.uint8, device=env.device)

    def kernel():
        env.search_rollout(K, eps=38 / 256, action_seed=1, trace=trace, end=end)

    def per_step(policy):
        def run():
            for k in range(K):
                env.actions(policy, action_seed=1, step=k, out=act, eps=38 / 256)
                env.step(act, autoreset=False, buffers=buf)
        return run

    legs = {"k_search_rollout": kernel, "per_step_heuristic": per_step("heuristic"),
            "per_step_eps_heuristic": per_step("eps_heuristic")}
    ms = {k: [] for k in legs}
    for rep in range(a.reps + 2):                      # two warm-up rounds
        for name, call in legs.items():
            env.restore(start)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            torch.cuda.synchronize()
            if rep >= 2:
                ms[name].append(e0.elapsed_time(e1))
    out = {"lanes": N, "books": a.books, "width": W, "orders": a.orders, "K": K, "reps": a.reps,
           "ms": {k: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in ms.items()}}
    env.restore(start)
    kernel()
    steps = end.steps.cpu().numpy()
    out["pass0_lane_steps"] = {"mean": float(steps.mean()), "min": int(steps.min()), "max": int(steps.max())}
    out["trace_bytes_per_step"] = 8 * N
    # (4) the whole search
    t0 = time.perf_counter()
    r = env.search(books, W, stride=a.stride, eps=38 / 256, action_seed=1)
    torch.cuda.synchronize()
    out["search"] = {"stride": a.stride, "wall_s": time.perf_counter() - t0, "passes": int(r["passes"]),
                     "solved_pass0": int((~np.isnan(r["history"][0])).sum()), "solved": int(r["solved"].sum()),
                     "improved_books": int((r["history"][-1] < r["history"][0]).sum()),
                     "mean_makespan_pass0_of_solved_at_pass0": float(np.nanmean(r["history"][0])),
                     "mean_makespan_end_of_solved_at_pass0":
                         float(np.nanmean(np.where(np.isnan(r["history"][0]), np.nan, r["history"][-1])))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
