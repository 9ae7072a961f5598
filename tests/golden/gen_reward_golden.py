"""Generate tests/golden/reward_weights.npz by running the REFERENCE under non-default reward weights.

TEST INFRASTRUCTURE, CPU only, in the style of gen_golden.py (whose reference import, stand-ins,
counter RNG and result encoding it reuses).  For every weight set of tests/parity_util.py
(DISTINCT, SCALED, GLOBAL_ONLY, LOCAL_ONLY) and each of the three policies (unmasked random,
masked random, the a2c heuristic) one reference env per seed runs STEPS steps with auto-reset after
``sim.reward_calculator``'s sixteen fields were set to the case's weights.  Recorded, and nothing
else: the sixteen weights of each set, the actions, the f64 rewards, the encoded action results,
term and trunc.  tests/test_oracle_golden.py replays the actions on the oracle under the same
weights; the rewards must be equal byte for byte.

The archive is written with fixed member dates, so a second run reproduces it byte for byte.

Usage:  python tests/golden/gen_reward_golden.py
"""
import contextlib
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import parity_util as P  # noqa: E402
from tests.golden import gen_golden as G  # noqa: E402

STEPS = 300
SEEDS = (1, 5)
POLICIES = (("unmasked", 30), ("masked", 30), ("heuristic", 3))   # (policy, orders per episode)
OUT = os.path.join(HERE, "reward_weights.npz")


def run(W, a2c_mod, weights, seed, policy, num_orders):
    env = W.FJSPParallelEnv()
    rc = env.simulation.reward_calculator
    for name, w in zip(P.REWARD_NAMES, weights):
        assert hasattr(rc, name), name
        setattr(rc, name, float(w))
    np.random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        obs, _ = env.reset(seed=seed, options={"num_orders": num_orders})
    heur = a2c_mod.MultiAgentA2C.__new__(a2c_mod.MultiAgentA2C) if policy == "heuristic" else None
    rec = {k: [] for k in ("actions", "rewards", "results", "term", "trunc")}
    for t in range(STEPS):
        if policy == "unmasked":
            act = G.action_rng(seed, seed, t)
        elif policy == "masked":
            act = G.action_rng(seed, seed, t, G.masks_of(obs))
        else:
            hd = heur._get_heuristic_actions(env.unwrapped.simulation)
            act = [hd[a] for a in G.AGENTS]
        with contextlib.redirect_stdout(io.StringIO()):
            obs, rew, term, trunc, info = env.step({a: int(act[i]) for i, a in enumerate(G.AGENTS)})
        assert env.simulation.reward_calculator is rc
        rec["actions"].append(np.array(act, np.uint8))
        rec["rewards"].append(np.array([rew[a] for a in G.AGENTS], np.float64))
        rec["results"].append(np.array([G.encode_result(a, info[a]["action_result"]) for a in G.AGENTS], np.uint32))
        te, tr = term[G.AGENTS[0]], trunc[G.AGENTS[0]]
        rec["term"].append(np.uint8(te))
        rec["trunc"].append(np.uint8(tr))
        if te or tr:
            with contextlib.redirect_stdout(io.StringIO()):
                obs, _ = env.reset(options={"num_orders": num_orders})
    return {k: np.stack(v) for k, v in rec.items()}


def save(path, arrays):
    """np.savez_compressed with fixed member dates (numpy stamps the members with the clock)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zi, buf.getvalue())


def main():
    W, a2c_mod, _ = G.import_reference()
    out = {}
    for sname, weights in P.REWARD_SETS.items():
        out[f"{sname}_weights"] = np.array(weights, np.float64)
        for policy, num_orders in POLICIES:
            for seed in SEEDS:
                tr = run(W, a2c_mod, weights, seed, policy, num_orders)
                for k, v in tr.items():
                    out[f"{sname}_{policy}_s{seed}_{k}"] = v
    save(OUT, out)


if __name__ == "__main__":
    main()
