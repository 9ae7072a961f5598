"""The CPU searches behind the status tests' constants (oracle alone; no GPU).

  python scripts/search_status_cases.py c-seed [LAST] [FIRST]
      action seeds FIRST..LAST (default 0..5999) of configuration C (parity_util.STATUS_CFGS, 200 envs x 260
      steps): prints those at which PROD_LOST appears in unflagged envs of at least 4 different
      16-env blocks under the random policy with nothing flagged, with the masked policy's figures
      (STATUS_CFGS["C"]["action_seed"] = 4602 is the first that meets both).
  python scripts/search_status_cases.py obs [TABLES] [KEEP]
      FJSP_STATUS_OBS_OVERFLOW inside a valid episode: order tables of seeds 0..TABLES-1 (default
      3 000 000; ~8 GB of memory), ranked by a lower bound on the steps any controller needs to
      queue 128 products of one colour (7 AGV actions per wanted tray, 3 per other tray, one
      product loaded per step); tests/overflow_scripts.py's controller then runs on the KEEP
      (default 2 500) most favourable tables, every colour.  Prints the fullest packaging queues
      (128 = the flag; overflow_scripts.OBS_SEED = 2 528 654 is the one table that reaches it).
  python scripts/search_status_cases.py blue2 [SEEDS]
      a configuration in which packaging_blue_2 earns its three reward terms (tests/test_gpu_rewards.py):
      432 configurations at action seed 13 under masked actions (200 envs x 280 steps), then action
      seeds 0..SEEDS-1 (default 400) on the best six; ranked by the smallest of the three counts on
      unflagged env-steps (parity_util.STATUS_CFGS["F"]: 31 / 161 / 68, nothing flagged)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O  # noqa: E402
from tests import overflow_scripts as S, parity_util as P  # noqa: E402


def c_seed(last=5999, first=0):
    c = P.STATUS_CFGS["C"]

    def stat(seed, policy):
        rec, _, _ = O.rollout(200, 260, seeds=P.status_seeds(200), num_orders=c["num_orders"], action_seed=seed,
                              policy=policy, **c["cfg"])
        st = rec["status"]
        fl = (st & 0x80000007) != 0
        pl = ((st & O.ST_PROD_LOST) != 0) & ~fl
        envs = np.nonzero(pl.any(0))[0]
        return int(pl.sum()), envs.tolist(), len(set((envs // 16).tolist())), int(fl.sum())
    for seed in range(first, last + 1):
        r0 = stat(seed, 0)
        if r0[2] >= 4 and r0[3] == 0:
            print(seed, "random (env-steps, envs, blocks, flagged)", r0, "masked", stat(seed, 1), flush=True)


def obs(tables=3000000, keep=2500):
    o = O.OracleEnv(**S.OBS_CFG)
    tab = np.zeros((tables, 64), np.uint32)
    for s in range(tables):
        o.reset(seed=s, num_orders=64)
        tab[s] = o.orders(64)
    n, col = (tab & 15).astype(np.int32), ((tab >> 6) & 3).astype(np.int32)
    trays, loaded = 1 + (n > 7), np.cumsum(n, 1)
    best = np.full(tables, 10**9)
    for c in (1, 2, 3):
        w = col == c
        need = np.maximum(np.cumsum(np.where(w, 7 * trays, 3 * trays), 1), loaded)
        reach = np.cumsum(np.where(w, n, 0), 1) >= 128
        first = np.where(reach.any(1), reach.argmax(1), -1)
        best = np.minimum(best, np.where(first >= 0, need[np.arange(tables), np.maximum(first, 0)], 10**9))
    print("tables whose lower bound fits an episode:", int((best <= 254).sum()), flush=True)
    top = []
    for s in np.argsort(best)[:keep]:
        for c in (1, 2, 3):
            _, recs = S.packaging_overflow_script(int(s), c, search=True)
            flagged = bool(recs[-1]["status"] & O.ST_OBS_OVERFLOW)
            top.append((128 if flagged else int(recs["obs_i8"][:, 5::2].max()), int(s), c, len(recs) - 1))
    top.sort(reverse=True)
    print("fullest queues (products, seed, colour, last step):", top[:12])


def blue2(nseeds=400):
    import itertools
    flags = O.ST_EXCEPTION | O.ST_OBS_OVERFLOW | O.ST_PKG_WAIT

    def score(cfg, aseed):
        rec, _, _ = O.rollout(200, 280, seeds=P.status_seeds(200), num_orders=20, action_seed=aseed, policy=1, **cfg)
        fl = (rec["status"] & flags) != 0
        c = P.reward_term_counts(rec, ~fl)
        b = (c["pkg_blue_2.start"], c["pkg_blue_2.complete"], c["pkg_blue_2.idle"])
        return min(b), b, float(fl.mean())
    res = []
    for cap, tc, ptp, pts, mx in itertools.product((1, 2, 3), (1, 2, 3), (250, 500, 1000, 2000), (10, 60), (200, 253)):
        cfg = dict(packaging_capacity=cap, tray_capacity=tc, mask_tray_capacity=tc, pt_packaging=ptp, pt_small=pts,
                   pt_big=pts if pts == 10 else 120, max_episode_steps=mx)
        res.append(score(cfg, 13) + (cfg,))
    res.sort(key=lambda r: (-r[0], r[2]))
    print("configurations at action seed 13 (min, (start, complete, idle), flagged share, cfg):")
    for r in res[:10]:
        print(" ", r, flush=True)
    out = []
    for r in res[:6]:
        out += [score(r[3], a) + (r[3], a) for a in range(nseeds)]
    out.sort(key=lambda r: (-r[0], r[2]))
    print("action seeds on the best six:")
    for r in out[:10]:
        print(" ", r, flush=True)


if __name__ == "__main__":
    cmd, args = (sys.argv[1] if len(sys.argv) > 1 else ""), [int(x) for x in sys.argv[2:]]
    if cmd == "c-seed":
        c_seed(*args)
    elif cmd == "obs":
        obs(*args)
    elif cmd == "blue2":
        blue2(*args)
    else:
        sys.exit(__doc__)
