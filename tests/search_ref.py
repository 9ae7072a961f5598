"""Oracle-side reference of the rollout search (TEST-ONLY): the perturbed heuristic composed in
Python from OracleEnv.heuristic(), oracle.actions() and the coin's formula, the lane loop driven
through OracleEnv.step, and the whole search over OracleEnvs (a committed state is reached by
replaying the action prefix from the seeded reset that draws the book)."""
import numpy as np

from oracle import oracle as OR

M64 = (1 << 64) - 1
COIN_MIX = 0x9E3779B97F4A7C15


def fmix64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def coins(seed, gid, step):
    """The eight coin bytes of (seed, gid, step): agent a takes the masked draw iff coins[a] < eps8."""
    h = fmix64((seed & M64) ^ fmix64(((gid & 0xFFFFFFFF) << 32) | (step & 0xFFFFFFFF)))
    h2 = fmix64(h ^ COIN_MIX)
    return np.array([(h2 >> (8 * a)) & 0xFF for a in range(8)], np.int64)


def eps_actions(ref, masks, seed, gid, step, eps8):
    """eps_heuristic_actions on an OracleEnv whose current masks are `masks`."""
    h = ref.heuristic()
    m = OR.actions(seed & M64, gid, step, masks)
    return np.where(coins(seed, gid, step) < eps8, m, h).astype(np.uint8)


class Lane:
    """One OracleEnv with the record of its last reset / step (the masks the policy reads)."""

    def __init__(self, seed, num_orders, prefix=()):
        self.ref = OR.OracleEnv()
        self.rec = self.ref.reset(seed=seed, num_orders=num_orders)
        for a in prefix:
            self.rec = self.ref.step(a)

    def book_words(self):
        return (self.ref.orders() & 0xFF).astype(np.uint32)

    def run(self, K, eps8, seed, gid, step0, script=None):
        """The lane loop of fjsp_search_rollout: returns (trace [n, 8], end dict)."""
        script = np.zeros((0, 8), np.uint8) if script is None else np.asarray(script, np.uint8).reshape(-1, 8)
        trace, end = [], {"steps": -1, "flags": 0, "orders_completed": 0, "packaged": 0, "sim_time": 0.0}
        for k in range(K):
            a = script[k] if k < len(script) else eps_actions(self.ref, self.rec["masks"], seed, gid, step0 + k, eps8)
            trace.append(np.array(a, np.uint8))
            self.rec = r = self.ref.step(a)
            end.update(orders_completed=int(r["orders_completed"]), packaged=int(r["packaged"]),
                       sim_time=float(r["sim_time"]))
            if r["term"] or r["trunc"]:
                end.update(steps=k + 1, flags=int(r["term"]) | (int(r["trunc"]) << 1))
                break
        return np.array(trace, np.uint8).reshape(-1, 8), end


def key_of(end):
    if end["flags"] & 1:
        return (0, end["sim_time"], 0)
    return (1, -end["orders_completed"], -end["packaged"])


def search_ref(cases, width, stride, eps8, action_seed, max_steps=200):
    """The search over OracleEnvs.  cases: [(seed, num_orders)] per book; lane i * width + r is
    replica r of book i.  Returns history [P, I], makespan [I], solved [I], actions (list [T_i, 8])."""
    K0, I = max_steps + 1, len(cases)
    incs = []
    for i, (s, k) in enumerate(cases):
        runs = [Lane(s, k).run(K0, eps8, action_seed, i * width + r, 0) for r in range(width)]
        best = min(range(width), key=lambda r: (key_of(runs[r][1]), r))
        incs.append({"actions": runs[best][0], "end": runs[best][1]})
    span = lambda inc: inc["end"]["sim_time"] if inc["end"]["flags"] & 1 else np.nan  # noqa: E731
    history = [[span(inc) for inc in incs]]
    p = 1
    while True:
        act = [i for i in range(I) if p * stride < len(incs[i]["actions"])]
        if not act:
            break
        d = p * stride
        for i in act:
            s, k = cases[i]
            inc = incs[i]
            runs = []
            for r in range(width):
                script = inc["actions"][d:] if r == 0 else None
                runs.append(Lane(s, k, prefix=inc["actions"][:d]).run(K0 - d, eps8, action_seed, i * width + r,
                                                                      (p << 12) + d, script))
            best = min(range(width), key=lambda r: (key_of(runs[r][1]), r))
            if key_of(runs[best][1]) < key_of(inc["end"]):
                incs[i] = {"actions": np.concatenate([inc["actions"][:d], runs[best][0]]), "end": runs[best][1]}
        history.append([span(inc) for inc in incs])
        p += 1
    return {"history": np.array(history, np.float64), "makespan": np.array([span(inc) for inc in incs]),
            "solved": np.array([bool(inc["end"]["flags"] & 1) for inc in incs]),
            "actions": [inc["actions"] for inc in incs]}
