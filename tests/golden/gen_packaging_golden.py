"""Generate tests/golden/packaging.npz by running the REFERENCE itself.

TEST INFRASTRUCTURE, like gen_schedule_golden.py (whose write_npz and tray_code it uses, with
gen_golden.py's helpers and stand-ins): runs only where the reference checkout exists.

Runs.  The twelve traces.npz runs are replayed from their recorded actions (every step's result
words and flags must equal the recording).  Their packaging stations see little (the heuristic
traces have 34 / 30 / 28 / 23 drops at packaging, the random ones 1-5, blue_2 is never used and no
batch holds two runs), so scripted policies are added: the reference heuristic's actions
(MultiAgentA2C._get_heuristic_actions) with the station rows 4..7 replaced, 1000 steps, seeds 0
and 1, 5 orders, the actions recorded:
  lazy12       START only where step-in-episode % 12 == 11, IDLE otherwise: several runs per batch
  eager_long   START every step, packaging time 100, max_episode_steps 60: overlapping batches,
               episode ends with a batch in flight
  lazy7_long   START where step-in-episode % 7 == 6, the same config: queued and in-flight runs at
               episode ends
  eager_cap5   (seed 0 only) START every step, packaging time 200, 8 orders, the stations' simpy
               Resource capacity set to 5 on the reference's objects after every reset (the
               reference hard-codes 20): blue_2 is used, and later drops find no station with room
               and their products are lost
The reference reads the packaging time at construction (constants.PROCESSING_TIMES), so it is set
before the env is built.

Written per run `<key>_`:
  actions  u8 [steps, 8]   results u32 [steps, 8]   term, trunc u8 [steps]   (scripted runs; the
           trace runs' are traces.npz's)
  cfg      i32 [4]         pt_packaging, max_episode_steps, packaging capacity, num_orders
  orders   u8 [episodes, num_orders, 3]   as schedule.npz
  held     u32 [steps, 3]  as schedule.npz
  packaged i32 [steps]     info total_products_packaged
  pack     u32 [steps, 4]  the pack words (include/fjsp.h) of the state after each step and before
           the reset, from the reference's objects: runs = the trays with a product in the
           station's product_queue or in flight (not yet packaged), pending = len(product_queue) +
           resource.count, completed = products_completed
  runs     i64 [n, 7]      RUN_COLS, one row per tray run in (step written, station, FIFO) order,
           from object events only (never from the pack or result words): a tray's products
           entering a station (add_tray on that station's object), leaving its product_queue
           (granted), is_packaged turning true, episode ends.  The products of a tray share all
           three steps (asserted).  drop = the step of the add_tray call

After writing the file the script asserts what it contains (at least one batch of >= 2 runs, one
pair of overlapping batches at one station, one episode end with a granted unfinished run and one
with an ungranted one, >= 20 finished runs per heuristic trace) and prints the counts.  Found, as
runs / finished, batches of >= 2 runs, overlapping pairs, granted unfinished, ungranted, blue_2:
  heuristic_s0..3  34/34, 30/30, 28/28, 22/22 with none of the rest (no batch holds two runs)
  unmasked, masked 1-5 runs each; masked_s1 has one ungranted run at an episode end
  lazy12_s0, _s1   38/37 and 34/33, batches 1 and 2, ungranted 1 and 1
  eager_long       19/15 and 25/21, overlaps 3 and 4, granted unfinished 4 and 4
  lazy7_long       19/13 and 25/18, batches 0 and 1, overlaps 3 and 3, granted unfinished 5 and 6,
                   ungranted 1 and 1
  eager_cap5_s0    33/30, overlaps 1, granted unfinished 3, one run at blue_2; the host build's
                   status over the run is PROD_LOST alone

Usage:  python tests/golden/gen_packaging_golden.py
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402
import gen_schedule_golden as GS  # noqa: E402

RUN_COLS = ("station", "finished", "granted", "episode_start", "tray", "start", "end", "drop")
STATIONS = GG.AGENTS[4:8]
TRACE_RUNS = GS.RUNS
SCRIPTED = [  # key, START period, pt_packaging, max_episode_steps, capacity, num_orders, seeds
    ("lazy12", 12, 30, 200, 20, 5, (0, 1)),
    ("eager_long", 1, 100, 60, 20, 5, (0, 1)),
    ("lazy7_long", 7, 100, 60, 20, 5, (0, 1)),
    ("eager_cap5", 1, 200, 200, 5, 8, (0,)),
]
STEPS = 1000


class Watch:
    """The run list of one episode from object events."""

    def __init__(self, sim, capacity):
        self.sim = sim
        self.trays = [[] for _ in STATIONS]   # per station, in arrival order: dict per tray run
        self.now = 0
        for s, name in enumerate(STATIONS):
            st = sim.agents[name]
            if capacity != 20:
                st.resource._capacity = capacity
            st.add_tray = self._hook(s, st, st.add_tray)

    def _hook(self, s, st, inner):
        def add_tray(tray):
            before = len(st.product_queue)
            inner(tray)
            ps = list(st.product_queue[before:])
            assert ps and [id(p) for p in ps] == [id(p) for p in tray.products]
            self.trays[s].append({"code": GS.tray_code(tray), "products": ps, "drop": self.now, "start": None})
        return add_tray

    def after_step(self, ln):
        """Grants and completions visible in the objects after step ln; returns the finished runs
        per station in FIFO order."""
        done = [[] for _ in STATIONS]
        for s, name in enumerate(STATIONS):
            queued = {id(p) for p in self.sim.agents[name].product_queue}
            keep = []
            for run in self.trays[s]:
                out = [id(p) not in queued for p in run["products"]]
                assert all(out) or not any(out), "a tray's products left the queue at different steps"
                if all(out) and run["start"] is None:
                    run["start"] = ln
                packed = [bool(p.is_packaged) for p in run["products"]]
                assert all(packed) or not any(packed), "a tray's products were packaged at different steps"
                if all(packed):
                    assert not keep, "a run finished before an earlier one of its station"
                    done[s].append(run)
                else:
                    keep.append(run)
            self.trays[s] = keep
        return done

    def pack_words(self):
        w = []
        for s, name in enumerate(STATIONS):
            st = self.sim.agents[name]
            w.append(len(self.trays[s]) | ((len(st.product_queue) + st.resource.count) << 8) | (st.products_completed << 20))
        return w


def run(W, a2c_mod, key, seed, num_orders, steps, recorded=None, period=None, pt=30, max_steps=200, capacity=20):
    import constants
    constants.PROCESSING_TIMES["packaging"] = pt
    loc_of = {pos: int(loc.value) for loc, pos in constants.LOCATION_POSITIONS.items()}
    cfg = dict(constants.CONFIG, max_episode_steps=max_steps)
    env = W.FJSPParallelEnv(config=cfg)
    np.random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        env.reset(seed=seed, options={"num_orders": num_orders})
    heur = a2c_mod.MultiAgentA2C.__new__(a2c_mod.MultiAgentA2C)

    def order_table(sim):
        return [(len(o.products), o.products[0].product_type.value, o.products[0].packaging_color.value)
                for o in sim.orders]
    sim = env.unwrapped.simulation
    watch = Watch(sim, capacity)
    orders = [order_table(sim)]
    rec = {k: [] for k in ("actions", "results", "term", "trunc", "held", "pack", "packaged")}
    runs, ln = [], 0
    for t in range(steps):
        sim = env.unwrapped.simulation
        if recorded is not None:
            act = [int(x) for x in recorded["actions"][t]]
        else:
            hd = heur._get_heuristic_actions(sim)
            act = [hd[a] for a in GG.AGENTS]
            for s in range(4):
                act[4 + s] = 1 if ln % period == period - 1 else 0
        watch.now = ln
        with contextlib.redirect_stdout(io.StringIO()):
            _, _, term, trunc, info = env.step({a: act[i] for i, a in enumerate(GG.AGENTS)})
        res = np.array([GG.encode_result(a, info[a]["action_result"]) for a in GG.AGENTS], np.uint32)
        te, tru = bool(term[GG.AGENTS[0]]), bool(trunc[GG.AGENTS[0]])
        if recorded is not None:
            assert (res == recorded["results"][t]).all(), (key, t)
            assert (te, tru) == (bool(recorded["term"][t]), bool(recorded["trunc"][t])), (key, t)
        agv = sim.agv
        loc = loc_of[tuple(agv.position)]
        holders = [(agv.carrying_tray, False), (sim.small_machine.current_tray, sim.small_machine.is_busy),
                   (sim.big_machine.current_tray, sim.big_machine.is_busy)]
        held = []
        for r, (tray, busy) in enumerate(holders):
            w = (GS.HOLDS | GS.tray_code(tray)) if tray is not None else 0
            held.append(w | (GS.BUSY if busy else 0) | ((loc << GS.LOC_SHIFT) if r == 0 else 0))
        done = watch.after_step(ln)
        rec["pack"].append(watch.pack_words())
        for s in range(4):
            for r in done[s]:
                assert r["start"] is not None
                runs.append((s, 1, 1, t - ln, r["code"], r["start"], ln, r["drop"]))
            if te or tru:
                for r in watch.trays[s]:
                    g = r["start"] is not None
                    runs.append((s, 0, int(g), t - ln, r["code"], r["start"] if g else -1, -1, r["drop"]))
        rec["actions"].append(act)
        rec["results"].append(res)
        rec["term"].append(te)
        rec["trunc"].append(tru)
        rec["held"].append(held)
        rec["packaged"].append(int(info[GG.AGENTS[0]]["total_products_packaged"]))
        ln += 1
        if te or tru:
            with contextlib.redirect_stdout(io.StringIO()):
                env.reset(options={"num_orders": num_orders})
            sim = env.unwrapped.simulation
            orders.append(order_table(sim))
            watch = Watch(sim, capacity)
            ln = 0
    out = {"actions": np.array(rec["actions"], np.uint8), "results": np.array(rec["results"], np.uint32),
           "term": np.array(rec["term"], np.uint8), "trunc": np.array(rec["trunc"], np.uint8),
           "held": np.array(rec["held"], np.uint32), "pack": np.array(rec["pack"], np.uint32),
           "packaged": np.array(rec["packaged"], np.int32), "orders": np.array(orders, np.uint8),
           "runs": np.array(runs, np.int64).reshape(-1, len(RUN_COLS)),
           "cfg": np.array([pt, max_steps, capacity, num_orders], np.int32)}
    return out


def contents(r):
    """What a run holds of the things the fixture is for."""
    c = {k: r["runs"][:, i] for i, k in enumerate(RUN_COLS)}
    fin = c["finished"] == 1
    multi = overlap = 0
    batches = {}
    for i in np.flatnonzero(c["granted"] == 1).tolist():
        batches.setdefault((int(c["station"][i]), int(c["episode_start"][i]), int(c["start"][i])), []).append(i)
    multi = sum(len(v) >= 2 for v in batches.values())
    dur = int(r["cfg"][0]) // 10
    keys = sorted(batches)
    for a, b in zip(keys, keys[1:]):
        overlap += a[:2] == b[:2] and b[2] - a[2] < dur
    return {"runs": len(fin), "finished": int(fin.sum()), "multi_run_batches": int(multi), "overlaps": int(overlap),
            "granted_unfinished": int(((c["granted"] == 1) & ~fin).sum()), "ungranted": int((c["granted"] == 0).sum()),
            "blue_2": int((c["station"] == 1).sum())}


def main():
    W, a2c_mod, _ = GG.import_reference()
    traces = np.load(os.path.join(HERE, "traces.npz"))
    out, found = {}, {}
    for policy, num_orders, seed in TRACE_RUNS:
        key = f"{policy}_s{seed}"
        tr = {k: traces[f"{key}_{k}"] for k in ("actions", "results", "term", "trunc")}
        r = run(W, a2c_mod, key, seed, num_orders, len(tr["actions"]), recorded=tr)
        found[key] = contents(r)
        for k in ("cfg", "orders", "held", "packaged", "pack", "runs"):
            out[f"{key}_{k}"] = r[k]
    for name, period, pt, max_steps, cap, num_orders, seeds in SCRIPTED:
        for seed in seeds:
            key = f"{name}_s{seed}"
            r = run(W, a2c_mod, key, seed, num_orders, STEPS, period=period, pt=pt, max_steps=max_steps, capacity=cap)
            found[key] = contents(r)
            for k, v in r.items():
                out[f"{key}_{k}"] = v
    for key, c in found.items():
        print(key, c, flush=True)
    GS.write_npz(os.path.join(HERE, "packaging.npz"), out)
    tot = {k: sum(c[k] for c in found.values()) for k in next(iter(found.values()))}
    assert tot["multi_run_batches"] >= 1, "no batch of two or more runs"
    assert tot["overlaps"] >= 1, "no pair of overlapping batches at one station"
    assert tot["granted_unfinished"] >= 1 and tot["ungranted"] >= 1, "an unfinished kind is missing at the episode ends"
    low = {k: c["finished"] for k, c in found.items() if k.startswith("heuristic") and c["finished"] < 20}
    assert not low, ("a heuristic trace has fewer than 20 finished runs", low)


if __name__ == "__main__":
    main()
