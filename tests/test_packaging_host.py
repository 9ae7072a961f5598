"""CPU checks of schedule.packaging_reference (the specification of fjsp_packaging_scan) against
tests/golden/packaging.npz, whose run lists come from the reference's object events, and of
check_packaging / arrivals on the same records.  Hand-built slabs cover each rule by itself."""
import numpy as np
import pytest

from tests import packaging_util as PU

S = PU.schedule
DROP = 0x80 | 1 | (1 << 4) | (1 << 5)       # the AGV's result word of a drop at packaging
START = 0x80 | 3                            # a station's started_packaging
HOLDS = 1 << 13


def code(order, first, count):
    return order | (first << 6) | (count << 10)


def word(runs, pending, completed):
    return runs | (pending << 8) | (completed << 20)


def scan_chunks(r, chunk):
    T = len(r["term"])
    state, parts = None, []
    for t0 in range(0, T, chunk):
        sl = slice(t0, t0 + chunk)
        recs, state = S.packaging_reference(r["results"][sl], r["held"][sl], r["pack"][sl], r["term"][sl], r["trunc"][sl],
                                            state=state, step0=t0)
        parts.append(recs)
    return np.concatenate(parts), state


@pytest.mark.parametrize("chunk", [100000, 37, 1])
@pytest.mark.parametrize("key", PU.KEYS)
def test_reference_equals_the_fixture(key, chunk):
    r = PU.run(key)
    want = PU.fixture_records(r["runs"])
    got, _ = scan_chunks(r, chunk)
    assert got.tobytes() == want.tobytes(), (len(got), len(want))


def test_the_fixture_holds_what_it_is_for():
    tot = {}
    for key in PU.KEYS:
        r = PU.run(key)
        for k, v in PU.contents(PU.fixture_records(r["runs"]), int(r["cfg"][0]) // 10).items():
            tot[k] = tot.get(k, 0) + v
        if key.startswith("heuristic"):
            assert (r["runs"][:, 1] == 1).sum() >= 20
    assert tot["multi"] >= 1 and tot["overlap"] >= 1 and tot["granted_unfinished"] >= 1 and tot["ungranted"] >= 1
    assert tot["blue_2"] >= 1


class Slab:
    """A hand-built one-env slab: rows of (agv result, agv held, {station: result}, {station: pack word}, end)."""

    def __init__(self):
        self.rows = []

    def row(self, agv=0x81, held=0, st=None, pack=None, end=False):
        prev = self.rows[-1][3] if self.rows and not self.rows[-1][4] else [0, 0, 0, 0]
        pk = list(prev)
        for s, w in (pack or {}).items():
            pk[s] = w
        self.rows.append((agv, held, dict(st or {}), pk, end))
        return self

    def scan(self, **kw):
        T = len(self.rows)
        res, held, pack = np.zeros((T, 8, 1), np.uint32), np.zeros((T, 3, 1), np.uint32), np.zeros((T, 4, 1), np.uint32)
        term, trunc = np.zeros((T, 1), np.uint8), np.zeros((T, 1), np.uint8)
        for t, (agv, h, st, pk, end) in enumerate(self.rows):
            res[t, 1, 0], held[t, 0, 0] = agv, h
            for s in range(4):
                res[t, 4 + s, 0] = st.get(s, 0x81)
                pack[t, s, 0] = pk[s]
            trunc[t, 0] = end
        return S.packaging_reference(res, held, pack, term, trunc, **kw)[0]


def fields(recs):
    d = S.pack_records_dict(recs)
    return [(int(d["station"][i]), bool(d["finished"][i]), bool(d["granted"][i]), int(recs["tray"][i]),
             int(d["start"][i]), int(d["end"][i])) for i in range(len(recs))]


A, B, C = code(1, 0, 2), code(2, 0, 3), code(3, 1, 1)


def test_arrival_and_start_in_one_row():
    s = Slab().row(held=HOLDS | A | (5 << 16))
    s.row(agv=DROP, held=5 << 16, st={2: START}, pack={2: word(1, 2, 0)})
    s.row().row().row(pack={2: word(0, 0, 2)})
    recs = s.scan(step0=100, env_gid0=7)
    assert fields(recs) == [(2, True, True, A, 1, 4)]
    assert recs["env_gid"][0] == 7 and recs["episode_start"][0] == 100 and recs["reserved"][0] == 0
    assert int(recs["info"][0]) == 6 | (1 << 8) | (1 << 9) | (5 << 16) | (5 << 20)


def test_two_batches_in_flight():
    s = Slab().row(held=HOLDS | A)
    s.row(agv=DROP, st={0: START}, pack={0: word(1, 2, 0)})          # batch 1 at step 1
    s.row(held=HOLDS | B)
    s.row(agv=DROP, st={0: START}, pack={0: word(2, 5, 0)})          # batch 2 at step 3, batch 1 in flight
    s.row(pack={0: word(1, 3, 2)})                                   # batch 1 completes at step 4
    s.row().row(pack={0: word(0, 0, 5)})                             # batch 2 at step 6
    assert fields(s.scan()) == [(0, True, True, A, 1, 4), (0, True, True, B, 3, 6)]


def test_three_runs_complete_in_one_row():
    s = Slab()
    pend = 0
    for k, c in enumerate((A, B, C)):
        s.row(held=HOLDS | c)
        pend += (c >> 10) & 7
        s.row(agv=DROP, pack={3: word(k + 1, pend, 0)})
    s.row(st={3: START}).row().row().row(pack={3: word(0, 0, 6)})
    assert fields(s.scan()) == [(3, True, True, A, 6, 9), (3, True, True, B, 6, 9), (3, True, True, C, 6, 9)]


def test_a_lost_drop_writes_nothing():
    s = Slab().row(held=HOLDS | A).row(agv=DROP).row(end=True)
    assert len(s.scan()) == 0


def test_episode_end_with_both_unfinished_kinds():
    s = Slab().row(held=HOLDS | A)
    s.row(agv=DROP, st={0: START}, pack={0: word(1, 2, 0)})
    s.row(held=HOLDS | B)
    s.row(agv=DROP, pack={0: word(2, 5, 0)}, end=True)
    s.row(held=HOLDS | C)                                            # the next episode starts clean
    s.row(agv=DROP, pack={1: word(1, 1, 0)}, end=True)
    recs = s.scan()
    assert fields(recs) == [(0, False, True, A, 1, -1), (0, False, False, B, -1, -1), (1, False, False, C, -1, -1)]
    assert recs["episode_start"].tolist() == [0, 0, 4]


def test_arrival_in_the_row_another_run_completes():
    s = Slab().row(held=HOLDS | A)
    s.row(agv=DROP, st={2: START}, pack={2: word(1, 2, 0)})
    s.row().row(held=HOLDS | B)
    s.row(agv=DROP, pack={2: word(1, 3, 2)})                         # A completes, B arrives: runs stays 1
    s.row(st={2: START}).row().row().row(pack={2: word(0, 0, 5)})
    assert fields(s.scan()) == [(2, True, True, A, 1, 4), (2, True, True, B, 5, 8)]


def _all_records():
    out = []
    for i, key in enumerate(PU.KEYS):
        r = PU.run(key)
        out.append((key, r, PU.fixture_records(r["runs"], env_gid=i)))
    return out


def test_check_packaging_accepts_the_fixture_and_rejects_bad_records():
    for key, r, recs in _all_records():
        cfg = {"pt_packaging": int(r["cfg"][0]), "step_size": 10}
        S.check_packaging(recs, cfg)
        S.check_packaging(S.pack_records_dict(recs), cfg)
    key, r, recs = _all_records()[PU.KEYS.index("lazy12_s0")]
    cfg = {"pt_packaging": 30, "step_size": 10}
    fin = np.flatnonzero((recs["info"] & 0x100) != 0)
    bad = recs.copy()
    bad["end"][fin[3]] += 1
    with pytest.raises(ValueError, match="lasts"):
        S.check_packaging(bad, cfg)
    # two finished runs of one station and episode, the later one moved before the earlier
    info = recs["info"].astype(np.int64)
    pair = next((a, b) for a, b in zip(fin, fin[1:]) if info[a] == info[b] and
                recs["episode_start"][a] == recs["episode_start"][b] and recs["start"][a] < recs["start"][b])
    bad = recs.copy()
    bad[[pair[0], pair[1]]] = recs[[pair[1], pair[0]]]
    with pytest.raises(ValueError, match="before the previous run's start"):
        S.check_packaging(bad, cfg)


def test_arrivals_against_the_fixture_drop_steps():
    checked = 0
    for key, r, recs in _all_records():
        ops, _ = S.schedule_reference(r["results"], r["held"], r["term"], r["trunc"], env_gid0=int(recs["env_gid"][0]) if len(recs) else 0)
        got = S.arrivals(ops, recs)
        assert got.tolist() == r["runs"][:, 7].tolist(), key
        d = S.pack_records_dict(recs)
        assert ((d["start"] >= got) | ~d["granted"]).all()
        checked += len(got)
    assert checked > 300
    assert S.arrivals(np.zeros(0, S.OP_DTYPE), PU.fixture_records(PU.run("lazy12_s0")["runs"])).tolist() == \
        [-1] * len(PU.run("lazy12_s0")["runs"])


def test_gantt_takes_the_packaging_records():
    r = PU.run("lazy12_s0")
    recs = PU.fixture_records(r["runs"])
    g = S.gantt(S.pack_records_dict(recs))
    assert sum(len(v["start"]) for v in g.values()) == len(recs)
    assert {k[2] for k in g} <= {4, 5, 6, 7}
    for v in g.values():
        fin = v["finished"]
        assert (v["end_time"][fin] - v["start_time"][fin] == 30.0).all()
