"""Generate tests/golden/orders.npz by running the REFERENCE itself on order books the caller
chose and on orders that arrive during an episode.

TEST INFRASTRUCTURE, like gen_golden.py (whose helpers and stand-ins it uses): runs only where the
reference checkout exists.  Every run is one FJSPSimulation (default config, stepped directly, so a
run goes on after its episode has terminated) and is written as `<run>_<field>`:

  meta      i64 [4]        seed (-1 none), num_orders of the seeded reset (0 with a book), policy
                           (0 masked-random keyed (seed 0, env 0, step), 1 heuristic), steps
  book      u8 [K, 3]      (products, type, colour) of the episode's orders after the reset
  init_*                   the flattened observation after the reset
  actions, obs_i32, obs_i8, obs_f32, masks, rewards, term, trunc, results, sim_time,
  orders_completed, packaged   one row per step (gen_golden.run_trace's fields)
  arrivals  i64 [n, 7]     generate_order calls: before step t, argument (0 = None), the order it
                           created (products, type, colour), its id, its arrival_time
  arr_*                    the flattened observation after each arrival
  rng_key u32 [n, 624], rng_pos i64 [n]   numpy's global MT19937 state after each arrival

(a) explicit books, installed by substituting the three draws of generate_order
    (np.random.randint / np.random.choice) during reset(num_orders=K): `one` a 1 x 1-product book,
    `nine` one 9-product order (two trays), `full` 64 orders; 120 masked-random steps each, and
    `one_heur`: the 1-order book under the heuristic until it terminates.
(b) `arrivals`: reset(seed, 1) and the heuristic; the reference's own unpatched generate_order()
    with the pickup queue empty and the station idle, generate_order(3) while an order is half
    loaded, and generate_order() after the episode has terminated, without a reset: term goes
    1 -> 0 and the run goes on to a second termination.

Usage:  python tests/golden/gen_orders_golden.py
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as GG  # noqa: E402
from gen_schedule_golden import write_npz  # noqa: E402

STEP_FIELDS = ["actions", "obs_i32", "obs_i8", "obs_f32", "masks", "rewards", "term", "trunc", "results", "sim_time",
               "orders_completed", "packaged"]
BOOKS = {
    "one": [(1, 2, 3)],
    "nine": [(9, 1, 2)],
    "full": [(1 + (5 * i + 2) % 9, 1 + i % 3, 1 + (i // 3 + i) % 3) for i in range(64)],
}


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


@contextlib.contextmanager
def draws_from(book):
    """generate_order's three draws (FJSPSimulation.py:107,111-112) answered from `book`."""
    queue = [v for order in book for v in order]
    randint, choice = np.random.randint, np.random.choice
    np.random.randint = lambda lo, hi: queue.pop(0)
    np.random.choice = lambda members: {m.value: m for m in members}[queue.pop(0)]
    try:
        yield
    finally:
        np.random.randint, np.random.choice = randint, choice
    assert not queue


def order_row(o):
    return (len(o.products), o.products[0].product_type.value, o.products[0].packaging_color.value)


class Recorder:
    def __init__(self, sim, obs, seed, num_orders, policy):
        self.sim, self.obs, self.policy = sim, obs, policy
        self.rec = {k: [] for k in STEP_FIELDS}
        self.arr = {k: [] for k in ("arrivals", "arr_i32", "arr_i8", "arr_f32", "arr_masks", "rng_key", "rng_pos")}
        f = GG.flatten_obs(obs)
        self.out = {"init_i32": f[0], "init_i8": f[1], "init_f32": f[2], "init_masks": f[3],
                    "book": np.array([order_row(o) for o in sim.orders], np.uint8).reshape(-1, 3)}
        self.meta = [seed, num_orders, policy]
        self.heur = None
        self.t = 0
        self.term = False

    def step(self, a2c_mod):
        if self.policy == 0:
            act = GG.action_rng(0, 0, self.t, GG.masks_of(self.obs))
        else:
            if self.heur is None:
                self.heur = a2c_mod.MultiAgentA2C.__new__(a2c_mod.MultiAgentA2C)
            hd = self.heur._get_heuristic_actions(self.sim)
            act = [hd[a] for a in GG.AGENTS]
        with quiet():
            obs, rew, term, trunc, info = self.sim.step({a: int(act[i]) for i, a in enumerate(GG.AGENTS)})
        f = GG.flatten_obs(obs)
        r, i0 = self.rec, info[GG.AGENTS[0]]
        r["actions"].append(np.array(act, np.uint8))
        r["obs_i32"].append(f[0]); r["obs_i8"].append(f[1]); r["obs_f32"].append(f[2]); r["masks"].append(f[3])
        r["rewards"].append(np.array([rew[a] for a in GG.AGENTS], np.float64))
        r["term"].append(np.uint8(term[GG.AGENTS[0]])); r["trunc"].append(np.uint8(trunc[GG.AGENTS[0]]))
        r["results"].append(np.array([GG.encode_result(a, info[a]["action_result"]) for a in GG.AGENTS], np.uint32))
        r["sim_time"].append(float(i0["sim_time"]))
        r["orders_completed"].append(int(i0["orders_completed"]))
        r["packaged"].append(int(i0["total_products_packaged"]))
        self.obs, self.term = obs, bool(term[GG.AGENTS[0]])
        self.t += 1

    def arrive(self, num_products=None):
        with quiet():
            o = self.sim.generate_order() if num_products is None else self.sim.generate_order(num_products)
        st = np.random.get_state()
        self.obs = self.sim.get_observations()
        f = GG.flatten_obs(self.obs)
        a = self.arr
        a["arrivals"].append(np.array([self.t, num_products or 0, *order_row(o), o.id, int(o.arrival_time)], np.int64))
        a["arr_i32"].append(f[0]); a["arr_i8"].append(f[1]); a["arr_f32"].append(f[2]); a["arr_masks"].append(f[3])
        a["rng_key"].append(np.asarray(st[1], np.uint32)); a["rng_pos"].append(np.int64(st[2]))

    def result(self):
        out = dict(self.out)
        out["meta"] = np.array(self.meta + [self.t], np.int64)
        for k, v in self.rec.items():
            out[k] = np.stack(v) if isinstance(v[0], np.ndarray) else np.array(v)
        if self.arr["arrivals"]:
            for k, v in self.arr.items():
                out[k] = np.stack(v)
        return out


def run_book(S, a2c_mod, book, policy, steps):
    sim = S.FJSPSimulation()
    with quiet(), draws_from(book):
        obs, _ = sim.reset(num_orders=len(book))
    R = Recorder(sim, obs, -1, 0, policy)
    assert R.out["book"].tolist() == [list(o) for o in book]
    while R.t < steps and not (policy == 1 and R.term):
        R.step(a2c_mod)
    return R


def run_arrivals(S, a2c_mod, seed, limit=190):
    sim = S.FJSPSimulation()
    with quiet():
        obs, _ = sim.reset(seed=seed, num_orders=1)
    R = Recorder(sim, obs, seed, 1, 1)
    pk = sim.pickup_station
    done = {"idle": False, "half": False, "after": False}
    terms = 0
    while R.t < limit and terms < 2:
        order = pk.current_order
        if not done["idle"] and R.t > 0 and order is None and not pk.order_queue and not R.term:
            R.arrive()
            done["idle"] = True
        elif done["idle"] and not done["half"] and order is not None and \
                0 < pk.current_order_product_idx < len(order.products):
            R.arrive(3)
            done["half"] = True
        elif done["half"] and not done["after"] and R.term:
            R.arrive()
            done["after"] = True
        was = R.term
        R.step(a2c_mod)
        terms += int(R.term and not was)
    return R, done, terms


def main():
    GG.import_reference()
    import FJSPSimulation as S
    import a2c as a2c_mod
    out = {}

    def put(name, R):
        r = R.result()
        print(f"{name}: {R.t} steps, {len(r['book'])} orders, term rows {int(np.sum(r['term']))}, "
              f"completed {int(r['orders_completed'][-1])}, arrivals {len(R.arr['arrivals'])}", flush=True)
        for k, v in r.items():
            out[f"{name}_{k}"] = v
    for name, book in BOOKS.items():
        put(name, run_book(S, a2c_mod, book, 0, 120))
    R = run_book(S, a2c_mod, BOOKS["one"], 1, 200)
    assert R.term, "the heuristic did not finish the one-order book"
    put("one_heur", R)
    for seed in range(64):   # the first seed whose run meets all three arrival states
        R, done, terms = run_arrivals(S, a2c_mod, seed)
        if all(done.values()) and terms == 2:
            break
    else:
        raise AssertionError("no seed gives the three arrival states and a second termination")
    r = R.result()
    t_after = int(r["arrivals"][2][0])
    assert r["term"][t_after - 1] == 1 and r["term"][t_after] == 0 and r["term"][-1] == 1
    put("arrivals", R)
    write_npz(os.path.join(HERE, "orders.npz"), out)


if __name__ == "__main__":
    main()
