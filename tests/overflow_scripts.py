"""Action scripts that reach the two guards no random policy reaches: FJSP_STATUS_OBS_OVERFLOW
(an int8 queue-length observation above 127) and FJSP_STATUS_SLOT_OVERFLOW (a 256th tray in one
episode).  TEST INFRASTRUCTURE; the oracle is the judge of both.

OBS_OVERFLOW is reachable inside a valid episode (max_episode_steps <= 253, so at most 254 steps),
barely: with tray_capacity 7, one-step machine runs and packaging stations that never start, a
greedy AGV controller that favours one colour queues the 128th product of that colour at step 248
of the most favourable of 3 000 000 order tables searched with the oracle alone (seed 2 528 654,
green; the runners-up end at 127).  A machine queue of 128 trays is not: it needs at least 3 AGV
actions per tray (pick, move, drop: 384 steps).
SLOT_OVERFLOW is not reachable inside an episode either: the pickup station opens at most one
tray per step, so an episode opens at most 254 of the arena's 255 slots.  It is reached only by a
caller that keeps stepping an env past its truncation without a reset (autoreset = 0, as
FJSPVecEnv.evaluate does when max_steps exceeds the episode length); slot_overflow_script does
that."""
import numpy as np

from oracle import oracle as O

# oracle locations (fjsp_oracle.c LOC_*) by grid position, and the AGV's move action to each
_LOC = {(0, 0): 1, (0, 3): 2, (2, 3): 3, (3, 0): 4, (3, 5): 5}   # PICKUP BIG SMALL STORAGE PACK
_MOVE = {1: 1, 3: 2, 2: 3, 4: 4, 5: 5}

OBS_CFG = dict(tray_capacity=7, mask_tray_capacity=7, max_episode_steps=253, pt_small=10, pt_big=10)
OBS_SEED, OBS_COLOUR, OBS_ORDERS = 2528654, 3, 64     # the search's best order table
SLOT_CFG = dict(tray_capacity=1, mask_tray_capacity=1, max_episode_steps=253)
SLOT_SEED, SLOT_ORDERS = 1, 64


def packaging_overflow_script(seed=OBS_SEED, colour=OBS_COLOUR, search=False):
    """Greedy controller on the oracle: the pickup station always loads, the machines start and
    signal as soon as they can, the packaging stations never start, and the AGV carries every tray
    of OBS_COLOUR through its machine to packaging (other trays, and one-product trays, go to
    storage; at the pickup station a waiting tray goes before a processed one elsewhere).  Stops
    at the step where the oracle flags ST_OBS_OVERFLOW, inside the first episode.  Returns
    (actions u8 [T, 8], the oracle's records of the T steps); the last record carries the flag.
    search=True (scripts/search_status_cases.py): any order table and colour; an episode that ends
    without the flag returns its records instead of failing."""
    cfg = OBS_CFG
    o = O.OracleEnv(**cfg)
    r = o.reset(seed=seed, num_orders=OBS_ORDERS)
    want = []
    for w in o.orders(64):
        n, c = int(w & 15), int((w >> 6) & 3)
        sizes = [7, n - 7] if n > 7 else [n]
        want += [c == colour and s > 1 for s in sizes]
    picked, carry_wanted, acts, recs = 0, False, [], []
    for _ in range(cfg["max_episode_steps"] + 1):
        I, q = r["obs_i32"], r["obs_i8"]
        a = np.zeros(8, np.uint8)
        a[0] = 1
        for m in (0, 1):
            mk = r["masks"][11 + 3 * m: 14 + 3 * m]
            a[2 + m] = 2 if mk[2] else (1 if mk[1] else 0)
        loc = _LOC.get((int(I[7]), int(I[8])), 0)
        if I[9]:
            if not carry_wanted:
                tgt = 4
            elif I[12]:
                ty = int(I[11])
                tgt = 3 if ty == 1 else 2 if ty == 3 else (3 if q[0] + q[1] <= q[2] + q[3] else 2)
            else:
                tgt = 5
            a[1] = 7 if loc == tgt else _MOVE[tgt]
        else:
            rs, rb = int(I[17]), int(I[18])
            if (loc == 3 and rs) or (loc == 2 and rb):
                a[1], carry_wanted = 6, True              # only wanted trays ever reach a machine
            elif loc == 1 and I[14]:
                a[1], carry_wanted = 6, want[picked]
                picked += 1
            elif rs or rb:
                a[1] = _MOVE[3] if rs >= rb else _MOVE[2]
            elif loc != 1:
                a[1] = _MOVE[1]
        acts.append(a)
        r = o.step(a)
        recs.append(r)
        if r["status"] & O.ST_OBS_OVERFLOW:
            return np.array(acts), np.array(recs)
        assert not r["status"] & (O.ST_EXCEPTION | O.ST_PKG_WAIT), "the script left the emulated path early"
        if search and (r["term"] or r["trunc"]):
            return np.array(acts), np.array(recs)
        assert not (r["term"] or r["trunc"]), "the episode ended before the queue overflowed"
    raise AssertionError("the oracle never flagged ST_OBS_OVERFLOW")


def slot_overflow_script(steps=258):
    """Trays of one product: the pickup station's LOAD opens, fills and hands over one tray per
    step, everything else idles.  The oracle has no slot arena and flags nothing; the kernels'
    arena (255 slots per episode) overflows at the 256th tray, i.e. at step index 255.  Returns
    (actions u8 [steps, 8], the oracle's records)."""
    o = O.OracleEnv(**SLOT_CFG)
    o.reset(seed=SLOT_SEED, num_orders=SLOT_ORDERS)
    assert int((o.orders(64) & 15).sum()) >= steps, "the order table must hold a product per step"
    a = np.zeros(8, np.uint8)
    a[0] = 1
    recs = [o.step(a) for _ in range(steps)]
    recs = np.array(recs)
    assert not recs["status"].any() and (recs["obs_i32"][:, 14] == np.arange(1, steps + 1)).all()
    return np.tile(a, (steps, 1)), recs


OBS_EXTRA = 12   # idle steps after the flag: through the truncation at step 253 into the next episode


def obs_overflow_case():
    """Three envs (seeds OBS_SEED - 1, OBS_SEED, OBS_SEED + 1): env 1 runs the packaging script and
    then idles through its truncation into the next episode, its neighbours idle throughout.
    Returns (actions u8 [T, 8, 3], the oracle's replay [T, 3], flag step)."""
    acts1, _ = packaging_overflow_script()
    T = len(acts1) + OBS_EXTRA
    acts = np.zeros((T, 8, 3), np.uint8)
    acts[:len(acts1), :, 1] = acts1
    seeds = np.array([OBS_SEED - 1, OBS_SEED, OBS_SEED + 1], np.uint32)
    judge, _, _ = O.rollout(3, T, seeds=seeds, num_orders=OBS_ORDERS,
                            actions_in=np.ascontiguousarray(acts.transpose(0, 2, 1)), **OBS_CFG)
    return acts, seeds, judge, len(acts1) - 1


def check_obs_overflow(status, obs_i8, ended, judge, tf):
    """status u32 [T, 3], obs_i8 [T, 3, 12], ended bool [T, 3] of a kernel's run of obs_overflow_case:
    the flag and its reason at the oracle's step, the wrapped int8, sticky to the truncation, the
    next episode clean, the neighbours untouched."""
    from tests import parity_util as P
    r = P.status_parity(status, judge, "obs overflow script", got_ended=ended)
    assert r["flagged_envs"] == 1 and not status[:, [0, 2]].any()
    assert not status[:tf, 1].any()
    assert status[tf, 1] == 0x3 and judge["status"][tf, 1] == (O.ST_OBS_OVERFLOW | O.ST_EXCEPTION)
    assert obs_i8[tf, 1].tobytes() == judge["obs_i8"][tf, 1].tobytes() and obs_i8[tf, 1, 11] == -128
    assert obs_i8[tf - 1, 1, 11] == 124
    trunc_at = OBS_CFG["max_episode_steps"]
    assert (status[tf:trunc_at + 1, 1] == 0x3).all() and ended[trunc_at, 1] and not ended[tf:trunc_at, 1].any()
    assert not status[trunc_at + 1:, 1].any() and len(status) > trunc_at + 3
    return r
