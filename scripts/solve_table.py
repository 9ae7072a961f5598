"""Best-of-K sampling as a solver, measured: makespans of five order books under the built-in
heuristic, under best-of-32 and best-of-1024 masked-random schedules (FJSPVecEnv.solve) and under
32 sampled rollouts of the trained checkpoint (tests/golden/trained_policy.npz).  The books are the
tables that seed 11 / 1 order, seed 11 / 2 orders, seed 0 / 2 orders, seed 3 / 5 orders and seed
7 / 5 orders draw.  Nothing is thresholded; the table is what came out.

usage: python scripts/solve_table.py [--out profiles/orders/solve.json]
"""
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
K = importlib.import_module("multi-agent-rl-for-fjsp_amd.kpis")
A = importlib.import_module("multi-agent-rl-for-fjsp_amd.a2c_vec")

CASES = [(11, 1), (11, 2), (0, 2), (3, 5), (7, 5)]
ACTION_SEED = 5


def drawn_books():
    books = []
    for seed, k in CASES:
        env = V.FJSPVecEnv(1)
        env.reset(seeds=[seed], num_orders=k)
        books.append(O.from_env_view(env.read_env(0)))
    return books


def num(x):
    return None if np.isnan(x) else float(x)


def sampled(books, samples):
    env = V.FJSPVecEnv(len(books) * samples)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = env.solve(books, samples, policy="masked", action_seed=ACTION_SEED)
    dt = time.perf_counter() - t0
    span = r["all_makespans"]
    return {"makespan": [num(x) for x in r["makespan"]], "solved": r["solved"].tolist(),
            "terminated_replicas": (~np.isnan(span)).sum(axis=1).tolist(),
            "median_terminated": [num(np.nanmedian(s)) if (~np.isnan(s)).any() else None for s in span],
            "wall_seconds": dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "orders", "solve.json"))
    args = ap.parse_args()
    books = drawn_books()
    I = len(books)
    words, counts = O.encode(books)
    steps = 201
    heur = V.FJSPVecEnv(I).evaluate_kpis(policy="heuristic", steps=steps, orders=words, counts=counts)
    h = K.best_of(heur["kpis"], 1, instances=I)
    out = {"cases": [{"seed": s, "num_orders": k, "book": b, "products": sum(o[0] for o in b)}
                     for (s, k), b in zip(CASES, books)],
           "steps": steps, "step_size": 10, "action_seed": ACTION_SEED,
           "heuristic": {"makespan": [num(x) for x in h["makespan"]], "solved": h["solved"].tolist()},
           "masked_best_of_32": sampled(books, 32), "masked_best_of_1024": sampled(books, 1024)}
    samples = 32
    L = A.VecMultiAgentA2C(V.FJSPVecEnv(64), batch_size=16, seed=1)
    L.load_state_dicts(A.load_npz_weights(os.path.join(REPO, "tests", "golden", "trained_policy.npz")))
    w32, c32 = O.encode([b for b in books for _ in range(samples)])
    res = L.evaluate_kpis(steps=steps, env=V.FJSPVecEnv(I * samples), deterministic=False, orders=w32, counts=c32)
    p = K.best_of(res["kpis"], samples, instances=I)
    out["trained_policy_sampled_best_of_32"] = {
        "makespan": [num(x) for x in p["makespan"]], "solved": p["solved"].tolist(),
        "terminated_replicas": (~np.isnan(p["all_makespans"])).sum(axis=1).tolist(),
        "best_orders_completed": p["records"]["orders_completed"].tolist()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
