"""Generate tests/golden/schedule.npz by replaying traces.npz on the REFERENCE itself.

TEST INFRASTRUCTURE, like gen_golden.py (whose helpers and stand-ins it uses): runs only where
the reference checkout exists.  The twelve traces.npz runs (seeds 0..3 x unmasked / masked /
heuristic with 2 orders, 1000 steps, auto-reset) are replayed from their recorded actions; every
step's result words and flags must equal the recorded ones.  Written per run `<policy>_s<seed>_`:

  held     u32 [1000, 3]  the held-tray words (include/fjsp.h) of the state after each step and
                          before the reset, built from the reference's objects: rows AGV
                          (agv.carrying_tray, agv.position through LOCATION_POSITIONS), small and
                          big machine (current_tray, is_busy); tray code = products[0].order_id |
                          products[0].id % 100 << 6 | len(products) << 10
  ops      i64 [n, 8]     the operations, derived from object events and not from the held words
                          or the result words: the tray object that enters / leaves current_tray /
                          carrying_tray, is_busy being down, episode ends.  Columns OPS_COLS, in
                          (step, resource) order
  orders   u8 [episodes, num_orders, 3]   (products, type, colour) of every episode's orders (for
                          replays that do not draw them)

After writing the file the script asserts what the fixture was specified to contain: per heuristic
trace at least 20 finished small-machine ops, 5 finished big-machine ops, 50 AGV pickup / drop pairs
and 10 episodes.  The reference's seeds 0 and 1 meet it (27 / 7 / 69 / 11 and 22 / 8 / 62 / 11);
seed 2 gives 14 / 14 / 57 / 10 and seed 3 gives 7 / 16 / 47 / 7, so the script ends on that assertion
with the (byte-identical) fixture written.

Usage:  python tests/golden/gen_schedule_golden.py
"""
import contextlib
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402

OPS_COLS = ("resource", "finished", "from_loc", "to_loc", "episode_start", "tray", "start", "end")
RUNS = [(p, n, s) for s in range(4) for p, n in (("unmasked", 30), ("masked", 30), ("heuristic", 2))]
HOLDS, BUSY, LOC_SHIFT = 1 << 13, 1 << 14, 16


def tray_code(tray):
    """order [0,6) | first product [6,10) | count [10,13); an empty tray is 0.  Every tray must be a
    contiguous run of one order's products."""
    ps = tray.products
    if not ps:
        return 0
    o, first = ps[0].order_id, ps[0].id % 100
    assert ps[0].id // 100 == o
    for i, p in enumerate(ps):
        assert p.order_id == o and p.id == o * 100 + first + i, "tray is not a run of one order's products"
    assert o < 64 and first < 16 and len(ps) < 8
    return o | (first << 6) | (len(ps) << 10)


def replay(W, policy, num_orders, seed, tr):
    from constants import LOCATION_POSITIONS
    loc_of = {pos: int(loc.value) for loc, pos in LOCATION_POSITIONS.items()}
    steps = len(tr["actions"])
    env = W.FJSPParallelEnv()
    np.random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        env.reset(seed=seed, options={"num_orders": num_orders})

    def order_table(sim):
        return [(len(o.products), o.products[0].product_type.value, o.products[0].packaging_color.value)
                for o in sim.orders]
    held = np.zeros((steps, 3), np.uint32)
    ops, orders = [], [order_table(env.unwrapped.simulation)]
    ln = 0
    last = [None, None, None]    # the tray object each resource held after the previous step
    open_op = [None, None, None]  # [tray code, from, start]
    for t in range(steps):
        sim = env.unwrapped.simulation
        actions = {a: int(tr["actions"][t][i]) for i, a in enumerate(GG.AGENTS)}
        with contextlib.redirect_stdout(io.StringIO()):
            _, _, term, trunc, info = env.step(actions)
        res = np.array([GG.encode_result(a, info[a]["action_result"]) for a in GG.AGENTS], np.uint32)
        te, tru = bool(term[GG.AGENTS[0]]), bool(trunc[GG.AGENTS[0]])
        assert (res == tr["results"][t]).all(), (policy, seed, t)
        assert (te, tru) == (bool(tr["term"][t]), bool(tr["trunc"][t])), (policy, seed, t)
        agv = sim.agv
        assert tuple(agv.position) in loc_of, "the AGV is between locations at a step boundary"
        loc = loc_of[tuple(agv.position)]
        holders = [(agv.carrying_tray, False, loc), (sim.small_machine.current_tray, sim.small_machine.is_busy, 3),
                   (sim.big_machine.current_tray, sim.big_machine.is_busy, 2)]
        for r, (tray, busy, at) in enumerate(holders):
            w = (HOLDS | tray_code(tray)) if tray is not None else 0
            held[t, r] = w | (BUSY if busy else 0) | ((loc << LOC_SHIFT) if r == 0 else 0)
            entered = tray is not None and tray is not last[r]
            if entered:
                open_op[r] = [tray_code(tray), at, ln]
            closes = (tray is None and last[r] is not None) if r == 0 else not busy
            if open_op[r] is not None and (closes or te or tru):
                code, frm, start = open_op[r]
                to = (at if closes else 0) if r == 0 else frm
                ops.append((1 + r, int(closes), frm, to, t - ln, code, start, ln if closes else -1))
                open_op[r] = None
            last[r] = tray
        ln += 1
        if te or tru:
            with contextlib.redirect_stdout(io.StringIO()):
                env.reset(options={"num_orders": num_orders})
            orders.append(order_table(env.unwrapped.simulation))
            ln, last, open_op = 0, [None, None, None], [None, None, None]
    still_open = sum(o is not None for o in open_op)
    return held, np.array(ops, np.int64).reshape(-1, len(OPS_COLS)), np.array(orders, np.uint8), still_open


def write_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps, so that the file regenerates byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    W, _, _ = GG.import_reference()
    traces = np.load(os.path.join(HERE, "traces.npz"))
    out, unfinished_random, empty_machine_ops, unmet = {}, 0, 0, []
    for policy, num_orders, seed in RUNS:
        key = f"{policy}_s{seed}"
        tr = {k: traces[f"{key}_{k}"] for k in ("actions", "results", "term", "trunc")}
        held, ops, orders, still_open = replay(W, policy, num_orders, seed, tr)
        col = {c: ops[:, i] for i, c in enumerate(OPS_COLS)}
        episodes = int((tr["term"] | tr["trunc"]).astype(bool).sum())
        counts = {}
        for r, name in ((1, "agv"), (2, "small"), (3, "big")):
            m = col["resource"] == r
            counts[name] = (int(m.sum()), int((m & (col["finished"] == 1)).sum()))
        empty_machine_ops += int(((col["resource"] >= 2) & ((col["tray"] >> 10) == 0)).sum())
        unfin = int((col["finished"] == 0).sum())
        print(f"{key}: episodes {episodes}, ops written/finished agv {counts['agv']} small {counts['small']} "
              f"big {counts['big']}, unfinished at an episode end {unfin}, open at the last row {still_open}", flush=True)
        if policy == "heuristic":   # the conditions the fixture was specified with; checked after it is written
            if not (counts["small"][1] >= 20 and counts["big"][1] >= 5 and counts["agv"][1] >= 50 and episodes >= 10):
                unmet.append((key, counts, episodes))
        else:
            unfinished_random += unfin
        assert len(orders) == episodes + 1
        out[f"{key}_held"], out[f"{key}_ops"], out[f"{key}_orders"] = held, ops, orders
    assert unfinished_random >= 1, "no op was open at an episode end of the masked / unmasked runs"
    print("machine ops on an empty tray:", empty_machine_ops)
    write_npz(os.path.join(HERE, "schedule.npz"), out)
    assert not unmet, ("a heuristic trace has fewer than 20 finished small-machine ops, 5 finished big-machine ops, "
                       "50 AGV pairs or 10 episodes", unmet)


if __name__ == "__main__":
    main()
