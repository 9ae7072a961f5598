"""What a PPO epoch costs next to an A2C update, on the same collected batch in one process.

N envs x T steps are collected once; then, interleaved for `reps` repetitions from the same
restored state (parameters and both Adam states): the A2C update() (VecMultiAgentA2C.update: the
baseline), the PPO update() with a synchronising mark after the per-batch work and after every
epoch, and the PPO update() without marks (its total as a user runs it).  Every leg is warmed
first; times are host-clock ms around work that ends in a device synchronise; medians with
min / max and the quartiles.

The claim to check: an epoch after the first does strictly less work than an A2C update (no keys,
sort, verify or coefficient pass), so its median must not exceed the A2C update's.

usage: python scripts/ppo_epochs.py [--envs 4096] [--steps 256] [--epochs 4] [--reps 12] [--out FILE]
"""
import argparse
import copy
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

A = importlib.import_module("multi-agent-rl-for-fjsp_amd.a2c_vec")
PPO = importlib.import_module("multi-agent-rl-for-fjsp_amd.ppo_vec")
ve = importlib.import_module("multi-agent-rl-for-fjsp_amd.vec_env")


def summary(v):
    v = np.asarray(v, dtype=np.float64)
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    return {"median": round(float(med), 3), "min": round(float(v.min()), 3), "max": round(float(v.max()), 3),
            "q1": round(float(q1), 3), "q3": round(float(q3), 3), "n": int(v.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ppo", "epochs.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ppo_epochs.py measures on the GPU: no device visible")
    N, T = args.envs, args.steps
    L = PPO.VecMultiAgentPPO(ve.FJSPVecEnv(N), batch_size=T, seed=0, ppo_epochs=args.epochs)
    L.reset(seeds=torch.arange(N), num_orders=25)
    L.collect()
    ret, adv = L.advantages()
    params = list(L.actors.parameters()) + list(L.critic.parameters())
    state = ([p.detach().clone() for p in params], copy.deepcopy(L.optim_actor.state_dict()),
             copy.deepcopy(L.optim_critic.state_dict()))

    def restore():
        with torch.no_grad():
            for p, s in zip(params, state[0]):
                p.copy_(s)
        L.optim_actor.load_state_dict(copy.deepcopy(state[1]))
        L.optim_critic.load_state_dict(copy.deepcopy(state[2]))
        L.repack()
        torch.cuda.synchronize()

    def timed(fn):
        restore()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def ppo_marked(out):
        clock = [0.0]

        def stage(name):
            torch.cuda.synchronize()
            now = time.perf_counter()
            out.setdefault(name, []).append((now - clock[0]) * 1e3)
            clock[0] = now
        L.ppo_stage = stage
        restore()
        clock[0] = time.perf_counter()
        L.update(ret, adv)
        stage("repack")
        L.ppo_stage = None

    t = {"a2c_update": [], "ppo_update": []}
    marks = {}
    for i in range(args.warmup + args.reps):
        keep = i >= args.warmup
        a = timed(lambda: A.VecMultiAgentA2C.update(L, ret, adv))
        m = {}
        ppo_marked(m)
        p = timed(lambda: L.update(ret, adv))
        if keep:
            t["a2c_update"].append(a)
            t["ppo_update"].append(p)
            for k, v in m.items():
                marks.setdefault(k, []).extend(v)
    b = PPO.PPOBatch(L._bufs["feats"][:T], L._bufs["masks"][:T], L._bufs["actions"], ret, adv, L.gidx, L.midx)
    res = {"envs": N, "steps": T, "samples": N * T, "ppo_epochs": args.epochs, "reps": args.reps,
           "warmup_reps": args.warmup, "device": torch.cuda.get_device_name(0),
           "groups_actors": b.ga.U, "groups_critic": b.gc.U, "head_kernel": bool(b.head_kernel),
           "unit": "ms, host clock around work ending in a device synchronise",
           "a2c_update": summary(t["a2c_update"]), "ppo_update_unmarked": summary(t["ppo_update"]),
           "ppo_prepare": summary(marks["prepare"]),
           "ppo_epoch": [summary(marks[f"epoch{k}"]) for k in range(args.epochs)],
           "ppo_repack": summary(marks["repack"])}
    later = [x for k in range(1, args.epochs) for x in marks[f"epoch{k}"]]
    if later:
        res["ppo_epoch_after_first"] = summary(later)
        res["epoch_after_first_over_a2c_update"] = round(res["ppo_epoch_after_first"]["median"] /
                                                         res["a2c_update"]["median"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
