"""Rollout search over caller-written order books (FJSPVecEnv.search).

A best-of-W first pass under the perturbed heuristic (policy "eps_heuristic", fjsp_actions_eps),
then rollout improvement: each pass commits the next `stride` steps of the incumbent (the best
complete run so far), runs W lanes from the committed state to the episode's end (lane 0 follows
the rest of the incumbent, the others the perturbed heuristic on fresh random streams) and keeps a
run only if it is strictly better.  So a book's incumbent never gets worse, and the result is never
worse than the first pass's best-of-W.  Not a beam: no state is forked by a progress key (greedy
progress misleads in this shop: DESIGN.md §4); only complete runs are compared.

Every lane's run is one launch of k_search_rollout (fjsp_search_rollout), which writes the 8 action
bytes per step and one end record per lane.  The selection rule and the incumbent bookkeeping below
are pure numpy and need no GPU.
"""
import numpy as np

PASS_SHIFT = 12   # the pass number sits above 12 bits of the action stream's step


def run_key(term, sim_time, orders_completed, packaged):
    """A complete run's rank under kpis.best_of's rule; a smaller key is a better run.  A terminated
    run beats one that is not; among terminated runs the least sim_time (the makespan); among the
    others the most orders completed, then the most products packaged."""
    if term:
        return (0, float(sim_time), 0)
    return (1, -int(orders_completed), -int(packaged))


def select(flags, sim_time, orders_completed, packaged):
    """The best lane of one book's W end records (arrays [W]; flags bit 0 = terminated): the lowest
    lane among equals."""
    keys = [run_key(int(f) & 1, s, o, p) for f, s, o, p in zip(flags, sim_time, orders_completed, packaged)]
    return min(range(len(keys)), key=lambda r: (keys[r], r))


class Incumbent:
    """The best complete run of one book so far: its actions uint8 [T, 8] and its end record."""

    def __init__(self, actions, flags, sim_time, orders_completed, packaged):
        self.actions = np.ascontiguousarray(actions, dtype=np.uint8).reshape(-1, 8)
        self.flags, self.sim_time = int(flags), float(sim_time)
        self.orders_completed, self.packaged = int(orders_completed), int(packaged)

    @property
    def solved(self):
        return bool(self.flags & 1)

    @property
    def makespan(self):
        return self.sim_time if self.solved else float("nan")

    @property
    def key(self):
        return run_key(self.solved, self.sim_time, self.orders_completed, self.packaged)

    def __len__(self):
        return len(self.actions)

    def offer(self, prefix_len, tail, flags, sim_time, orders_completed, packaged):
        """A pass's best run from depth prefix_len: replaces the incumbent only if it is strictly
        better; its sequence is the committed prefix plus its trace.  Returns whether it did."""
        if not run_key(int(flags) & 1, sim_time, orders_completed, packaged) < self.key:
            return False
        tail = np.ascontiguousarray(tail, dtype=np.uint8).reshape(-1, 8)
        self.actions = np.concatenate([self.actions[:prefix_len], tail])
        self.flags, self.sim_time = int(flags), float(sim_time)
        self.orders_completed, self.packaged = int(orders_completed), int(packaged)
        return True


def book_active(inc, p, stride):
    """Whether pass p (depth d = p * stride) still has something to search for the book: a book is
    finished when the committed depth reaches its incumbent's length."""
    return p * stride < len(inc)


def history_monotone(history):
    """history [P, I] never increases per book (NaN = unsolved, which only comes first)."""
    h = np.asarray(history, dtype=np.float64)
    for col in h.T:
        seen = None
        for v in col:
            if np.isnan(v):
                if seen is not None:
                    return False
                continue
            if seen is not None and v > seen:
                return False
            seen = v
    return True


def search(env, books, width, stride=8, eps=0.15, action_seed=0, max_passes=None, packaging=False):
    """FJSPVecEnv.search.  env.num_envs must be len(books) * width; lane i * width + r is replica r of
    books[i].  max_passes: the most passes run, pass 0 included (None: until every book is finished).

    Returns solved [I], makespan [I] (NaN where unsolved), actions (list of uint8 [T_i, 8]), history
    [P, I] (the incumbent's makespan after each pass), passes = P, and "kpis" (the incumbents' KPI
    records [I]), "ops" (and "pack_ops" with packaging=True) from replaying the incumbents through
    evaluate_script: lane i * width replays book i's sequence, the other lanes idle."""
    import torch

    from . import orders as O
    from . import schedule as S
    from .vec_env import SearchEnd, eps8_of
    books, W, stride = [list(b) for b in books], int(width), int(stride)
    I, N = len(books), env.num_envs
    if W < 1 or I < 1 or N != I * W:
        raise ValueError(f"search needs num_envs == len(books) * width, got {N} envs for {I} books x {W} lanes")
    if stride < 1:
        raise ValueError("stride must be at least 1")
    K0 = int(env.config.max_episode_steps) + 1
    if K0 > (1 << PASS_SHIFT) - 1:
        raise ValueError(f"max_episode_steps + 1 = {K0} > 4095: the pass number is packed above 12 bits of the step")
    if max_passes is not None and int(max_passes) < 1:
        raise ValueError("max_passes must be at least 1 (pass 0 is the best-of-width run)")
    eps8_of(eps)
    words, counts = O.encode([b for b in books for _ in range(W)])
    dev = env.device
    trace = torch.zeros(K0, 8, N, dtype=torch.uint8, device=dev)
    end = SearchEnd(N, dev)

    def candidates(active_books):
        """Per active book the best lane of the launch just run: (lane, end fields, its trace)."""
        r = end.numpy()
        out = {}
        for i in active_books:
            sl = slice(i * W, (i + 1) * W)
            if (r["steps"][sl] < 1).any():
                raise RuntimeError(f"search: a lane of book {i} did not reach its episode's end")
            out[i] = i * W + select(r["flags"][sl], r["sim_time"][sl], r["orders_completed"][sl], r["packaged"][sl])
        lanes = torch.as_tensor([out[i] for i in active_books], device=dev, dtype=torch.long)
        cols = trace[:, :, lanes].cpu().numpy()                               # [K0, 8, n]
        return {i: (e, {k: r[k][e] for k in r}, cols[:r["steps"][e], :, j]) for j, (i, e) in enumerate(out.items())}

    # ---- pass 0: best-of-W from the reset
    env.reset_orders(words, counts)
    committed = env.snapshot()
    env.search_rollout(K0, eps=eps, action_seed=action_seed, step_base=0, t0=0, trace=trace, end=end)
    incs = []
    for i, (e, r, tr) in sorted(candidates(range(I)).items()):
        incs.append(Incumbent(tr, r["flags"], r["sim_time"], r["orders_completed"], r["packaged"]))
    history = [[inc.makespan for inc in incs]]
    # ---- passes p >= 1
    script = torch.zeros(K0, 8, N, dtype=torch.uint8, device=dev)
    p = 1
    while max_passes is None or p < int(max_passes):
        act_books = [i for i in range(I) if book_active(incs[i], p, stride)]
        if not act_books:
            break
        d = p * stride
        active = np.zeros(N, np.uint8)
        for i in act_books:
            active[i * W:(i + 1) * W] = 1
        # 1. commit: the incumbent's steps [d - stride, d) in every lane of the book, from the committed state
        host = np.zeros((stride, 8, N), np.uint8)
        for i in act_books:
            host[:, :, i * W:(i + 1) * W] = incs[i].actions[d - stride:d, :, None]
        script[:stride].copy_(torch.from_numpy(host))
        env.restore(committed)
        env.search_rollout(stride, eps=eps, action_seed=action_seed, step_base=p << PASS_SHIFT, t0=d - stride,
                           script=script[:stride], active=active, trace=trace, end=end)
        committed = env.snapshot(out=committed)
        # 2. W lanes to the episode's end: lane 0 the rest of the incumbent, the others the policy
        L = max(len(incs[i]) - d for i in act_books)
        host = np.zeros((L, 8, N), np.uint8)
        slen = np.zeros(N, np.int32)
        for i in act_books:
            rest = incs[i].actions[d:]
            host[:len(rest), :, i * W] = rest
            slen[i * W] = len(rest)
        script[:L].copy_(torch.from_numpy(host))
        env.search_rollout(K0 - d, eps=eps, action_seed=action_seed, step_base=p << PASS_SHIFT, t0=d, script=script[:L],
                           script_len=slen, active=active, trace=trace, end=end)
        for i, (e, r, tr) in candidates(act_books).items():
            incs[i].offer(d, tr, r["flags"], r["sim_time"], r["orders_completed"], r["packaged"])
        history.append([inc.makespan for inc in incs])
        p += 1
    # ---- replay the incumbents for their KPIs and per-operation schedules
    T = max(len(inc) for inc in incs)
    replay = np.zeros((T, 8, N), np.uint8)
    for i, inc in enumerate(incs):
        replay[:len(inc), :, i * W] = inc.actions
    rr = env.evaluate_script(torch.from_numpy(replay), words, counts, packaging=packaging)
    krec = rr["kpis"]["records"]
    win = np.arange(I) * W + env.env_id_base
    firsts = krec[(krec["end_step"] == krec["length"]) & np.isin(krec["env_gid"], win)]
    firsts = firsts[np.argsort(firsts["env_gid"])]
    makespan = np.array([inc.makespan for inc in incs])
    solved = np.array([inc.solved for inc in incs])
    if len(firsts) != I or (firsts["length"] != [len(inc) for inc in incs]).any():
        raise RuntimeError("search: the replay of the incumbents did not end where the search's runs did")
    if not np.array_equal(np.where(solved, firsts["makespan"], np.nan), makespan, equal_nan=True):
        raise RuntimeError(f"search: replayed makespans {firsts['makespan'].tolist()} differ from the searched "
                           f"{makespan.tolist()}")
    out = {"solved": solved, "makespan": makespan, "actions": [inc.actions.copy() for inc in incs],
           "history": np.array(history, dtype=np.float64), "passes": len(history), "kpis": firsts}
    for name, as_dict in (("ops", S.records_dict), ("pack_ops", S.pack_records_dict)):
        if name in rr:
            recs = rr[name]["records"]
            keep = np.isin(recs["env_gid"], win) & (recs["episode_start"] == 0)
            out[name] = as_dict(recs[keep], rr[name]["dropped"])
    return out


__all__ = ["search", "select", "run_key", "Incumbent", "book_active", "history_monotone", "PASS_SHIFT"]
