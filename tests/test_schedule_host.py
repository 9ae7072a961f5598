"""Per-operation schedules on the host: schedule_reference (the specification of
fjsp_schedule_scan) on hand-built slabs and against the operation lists the fixture derived from
the reference's objects, gantt / check, the record's layout and the entries' argument validation
(no GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import episodes_util as U
from tests import gpu_util as G
from tests import schedule_util as SU

S = SU.schedule
HOLDS, BUSY = S.HELD_HOLDS, S.HELD_BUSY
START, PICK, DROP = 0x83, 0x89, 0x91      # result words: executed | success | started / pickup / drop
CODE = 5 | (2 << 6) | (3 << 10)           # order 5, first product 2, 3 products
EMPTY = 0


def slab(T, N=1):
    return {"results": np.zeros((T, 8, N), np.uint32), "held": np.zeros((T, 3, N), np.uint32),
            "term": np.zeros((T, N), np.uint8), "trunc": np.zeros((T, N), np.uint8)}


def ref(s, lo=0, hi=None, **kw):
    hi = len(s["term"]) if hi is None else hi
    return S.schedule_reference(s["results"][lo:hi], s["held"][lo:hi], s["term"][lo:hi], s["trunc"][lo:hi], **kw)


def machine_run(s, m, t0, t1, code, e=0):
    """START of machine m at row t0, busy through row t1 - 1, the tray waiting (not busy) from t1."""
    s["results"][t0, 2 + m, e] = START
    s["held"][t0:t1, 1 + m, e] = HOLDS | BUSY | code
    s["held"][t1:, 1 + m, e] = HOLDS | code


def fields(recs):
    d = S.records_dict(recs)
    return [tuple(int(d[k][i]) for k in ("resource", "finished", "order", "first", "count", "start", "end", "from_loc",
                                         "to_loc", "episode_start")) for i in range(len(recs))]


def test_open_and_close():
    s = slab(12)
    machine_run(s, 0, 2, 8, CODE)
    s["held"][:, 0, 0] = 1 << 16
    s["results"][3, 1, 0] = PICK
    s["held"][3:6, 0, 0] = HOLDS | CODE | (1 << 16)
    s["held"][6:, 0, 0] = 3 << 16
    s["results"][6, 1, 0] = DROP
    recs, carry = ref(s, step0=40, env_gid0=9)
    assert fields(recs) == [(1, 1, 5, 2, 3, 3, 6, 1, 3, 40), (2, 1, 5, 2, 3, 2, 8, 3, 3, 40)]
    assert recs["env_gid"].tolist() == [9, 9] and not recs["reserved"].any()
    assert carry[:, 0].tolist() == [12, 0, 0, 0, 0, 0, 0]


def test_empty_tray_ends_where_it_starts():
    s = slab(4)
    s["results"][1, 3, 0] = START
    s["held"][1:, 2, 0] = HOLDS | EMPTY      # an empty tray's loop body never runs: never busy
    recs, _ = ref(s)
    assert fields(recs) == [(3, 1, 0, 0, 0, 1, 1, 2, 2, 0)]


def test_op_open_across_two_calls():
    s = slab(10)
    machine_run(s, 1, 1, 7, CODE)
    whole, carry_w = ref(s)
    a, carry = ref(s, 0, 4)
    assert len(a) == 0 and carry[:, 0].tolist() == [4, 0, 0, 0, 0, 1 | (CODE << 1) | (2 << 16), 1]
    b, carry = ref(s, 4, 10, carry=carry, step0=4)
    assert b.tobytes() == whole.tobytes() and fields(b) == [(3, 1, 5, 2, 3, 1, 7, 2, 2, 0)]
    assert carry.tobytes() == carry_w.tobytes() and carry.dtype == np.int32 and carry.shape == (S.CARRY_WORDS, 1)


def test_unfinished_at_episode_end():
    s = slab(9)
    machine_run(s, 0, 1, 9, CODE)
    s["results"][2, 1, 0] = PICK
    s["held"][2:5, 0, 0] = HOLDS | CODE | (4 << 16)
    s["trunc"][4, 0] = 1
    s["held"][5:, :, 0] = 0                   # the reset env
    s["held"][5:, 0, 0] = 1 << 16
    recs, carry = ref(s, step0=100)
    assert fields(recs) == [(1, 0, 5, 2, 3, 2, -1, 4, 0, 100), (2, 0, 5, 2, 3, 1, -1, 3, 3, 100)]
    assert carry[:, 0].tolist() == [4, 0, 0, 0, 0, 0, 0]
    # the next episode's ops count from its own start
    s["results"][6, 2, 0] = START
    s["held"][6, 1, 0] = HOLDS | BUSY | CODE
    s["held"][7:, 1, 0] = HOLDS | CODE
    recs, _ = ref(s, step0=100)
    assert fields(recs)[2] == (2, 1, 5, 2, 3, 1, 2, 3, 3, 105)


def test_start_in_the_row_after_a_close():
    s = slab(12)
    machine_run(s, 0, 0, 6, CODE)
    other = 6 | (1 << 10)
    s["results"][7, 2, 0] = START             # the close is row 6's, the next START row 7's
    s["held"][7:9, 1, 0] = HOLDS | BUSY | other
    s["held"][9:, 1, 0] = HOLDS | other
    recs, _ = ref(s)
    assert fields(recs) == [(2, 1, 5, 2, 3, 0, 6, 3, 3, 0), (2, 1, 6, 0, 1, 7, 9, 3, 3, 0)]
    S.check(recs, {"step_size": 10, "pt_small": 20, "pt_big": 120})


def test_rows_are_ordered_by_step_env_resource():
    s = slab(5, N=3)
    for e in (2, 0):
        machine_run(s, 1, 0, 2, CODE, e)     # closes in row 2
        machine_run(s, 0, 1, 3, CODE, e)     # closes in row 3, with the AGV's drop
        s["results"][0, 1, e] = PICK
        s["held"][0:3, 0, e] = HOLDS | CODE | (1 << 16)
        s["results"][3, 1, e] = DROP
    s["term"][3, 1] = 1
    s["results"][2, 1, 1] = PICK
    s["held"][2:, 0, 1] = HOLDS | CODE | (2 << 16)
    recs, _ = ref(s)
    d = S.records_dict(recs)
    assert list(zip(d["env"].tolist(), d["resource"].tolist())) == [(0, 3), (2, 3), (0, 1), (0, 2), (1, 1), (2, 1), (2, 2)]
    assert d["finished"].tolist() == [True] * 4 + [False, True, True]


@pytest.mark.parametrize("policy,seed", SU.RUNS)
def test_reference_equals_the_fixture_ops(policy, seed):
    """The scan over the fixture's result words and held words against the op list the fixture
    derived from object events, whole and in chunks of 37 rows with the carry passed on."""
    r = SU.run(policy, seed)
    want = SU.fixture_records(r["ops"])
    whole, carry_w = ref(r)
    assert whole.tobytes() == want.tobytes()
    assert len(want) > 0 and (want["info"] & S.INFO_FINISHED).any()
    parts, carry = [], None
    for lo, hi in U.cuts(1000, 37):
        p, carry = ref(r, lo, hi, carry=carry, step0=lo)
        parts.append(p)
    assert np.concatenate(parts).tobytes() == want.tobytes()
    assert carry.tobytes() == carry_w.tobytes()


def test_the_fixture_is_not_empty():
    """What the twelve runs hold, counted from the fixture alone: finished ops on both machines and
    AGV pairs in every heuristic run, ops open at an episode end in the random runs."""
    unfinished = 0
    for policy, seed in SU.RUNS:
        ops = SU.run(policy, seed)["ops"]
        res, fin = ops[:, 0], ops[:, 1]
        if policy == "heuristic":
            assert ((res == 1) & (fin == 1)).sum() >= 40 and ((res == 2) & (fin == 1)).sum() >= 5
            assert ((res == 3) & (fin == 1)).sum() >= 5
        else:
            unfinished += int((fin == 0).sum())
    assert unfinished >= 1


def test_gantt_and_check():
    r = SU.run("heuristic", 0)
    recs = SU.fixture_records(r["ops"])
    cfg = G.native.default_config()
    S.check(recs, cfg)
    S.check(S.records_dict(recs), None)
    g = S.gantt(recs, cfg)
    assert sum(len(v["start"]) for v in g.values()) == len(recs)
    for (env, es, res), v in g.items():
        assert env == 0 and res in (1, 2, 3)
        assert (np.diff(v["start"]) >= 0).all()
        assert (v["start_time"] == v["start"] * 10.0).all()
        assert (v["end_time"][v["finished"]] == v["end"][v["finished"]] * 10.0).all()
        assert np.isnan(v["end_time"][~v["finished"]]).all()
    small = g[(0, 0, 2)]
    assert (small["end"] - small["start"] == small["count"] * 6).all()
    # a doctored overlap and a wrong duration
    m = np.nonzero((recs["info"] & 0xFF) == 2)[0]
    bad = recs.copy()
    bad["start"][m[1]] = bad["start"][m[0]] + 1
    bad["end"][m[1]] = bad["start"][m[1]] + (bad["end"][m[1]] - recs["start"][m[1]])
    with pytest.raises(ValueError, match="after the next op's start"):
        S.check(bad, cfg)
    bad = recs.copy()
    bad["end"][m[0]] += 1
    with pytest.raises(ValueError, match="products need"):
        S.check(bad, cfg)
    a = np.nonzero((recs["info"] & 0xFF) == 1)[0]
    bad = recs.copy()
    bad["end"][a[0]] = recs["start"][a[1]] + 1
    with pytest.raises(ValueError, match="after the next op's start"):
        S.check(bad, cfg)


class _Rec(ctypes.Structure):   # include/fjsp.h fjsp_op_rec, field for field
    _fields_ = [("env_gid", ctypes.c_uint32), ("info", ctypes.c_uint32), ("episode_start", ctypes.c_int64),
                ("tray", ctypes.c_uint32), ("start", ctypes.c_int32), ("end", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


def test_record_layout_matches_the_header():
    hdr = open(os.path.join(G.REPO, "include", "fjsp.h")).read()
    size = int(re.search(r"#define\s+FJSP_OP_REC_BYTES\s+(\d+)", hdr).group(1))
    assert size == 32 == S.OP_DTYPE.itemsize == ctypes.sizeof(_Rec)
    body = re.search(r"typedef struct fjsp_op_rec \{(.*?)\} fjsp_op_rec;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])*;", body)
    assert names == list(S.OP_DTYPE.names) == [f[0] for f in _Rec._fields_]
    for f in names:
        assert S.OP_DTYPE.fields[f][1] == getattr(_Rec, f).offset, f
    assert {"fjsp_schedule_scan", "fjsp_schedule_temp_bytes", "fjsp_schedule_carry_words", "fjsp_step_held",
            "fjsp_actions"} <= set(G.native.EXPORTS)
    assert re.search(r"#define\s+FJSP_ABI_VERSION\s+14\b", hdr)
    assert G.native.lib().fjsp_abi_version() == 14
    for name, v in (("FJSP_HELD_CODE_MASK", S.HELD_CODE_MASK), ("FJSP_HELD_HOLDS", HOLDS), ("FJSP_HELD_BUSY", BUSY),
                    ("FJSP_HELD_LOC_SHIFT", S.HELD_LOC_SHIFT), ("FJSP_HELD_ROWS", S.HELD_ROWS)):
        assert int(re.search(r"#define\s+%s\s+(\w+?)u?\s" % name, hdr).group(1), 0) == v, name


def test_schedule_entries_validate_arguments_without_gpu():
    """fjsp_schedule_scan / _temp_bytes reject empty shapes, a slab past 2^30 positions, a negative
    capacity, null buffers, misaligned buffers and a short temp buffer before any launch;
    fjsp_step_held and fjsp_actions reject a null handle and null buffers."""
    L = G.native.lib()
    assert L.fjsp_schedule_carry_words() == S.CARRY_WORDS
    P = ctypes.c_void_p
    a = P(1 << 20)
    n = ctypes.c_uint64()
    assert L.fjsp_schedule_temp_bytes(256, 4096, ctypes.byref(n)) == 0
    need = n.value
    assert need == 256 * 64 * 4 + 16 and S.temp_bytes(256, 4096) == need
    for T, N in ((0, 8), (8, 0), (-1, 8)):
        assert L.fjsp_schedule_temp_bytes(T, N, ctypes.byref(n)) < 0 and b"must be > 0" in L.fjsp_last_error()
    assert L.fjsp_schedule_temp_bytes(8, 8, None) < 0 and b"null" in L.fjsp_last_error()
    assert L.fjsp_schedule_temp_bytes(1 << 20, 1 << 11, ctypes.byref(n)) < 0 and b"2^30" in L.fjsp_last_error()
    #     res held term trunc T    N     gid step carry recs cap count temp bytes stream
    ok = [a, a, a, a, 256, 4096, 0, 0, a, a, 100, a, a, need, None]

    def bad(i, v, msg):
        b = list(ok)
        b[i] = v
        assert L.fjsp_schedule_scan(*b) < 0 and msg in L.fjsp_last_error(), (i, v, L.fjsp_last_error())
    for i in (0, 1, 2, 3, 8, 9, 11, 12):
        bad(i, None, b"null")
    bad(4, 0, b"must be > 0")
    bad(4, -3, b"must be > 0")
    bad(5, 0, b"must be > 0")
    bad(10, -1, b"cap must be >= 0")
    bad(13, need - 1, b"temp buffer too small")
    bad(13, 0, b"temp buffer too small")
    bad(9, P((1 << 20) + 8), b"16-byte aligned")
    bad(12, P((1 << 20) + 4), b"16-byte aligned")
    for i in (0, 1, 8):
        bad(i, P((1 << 20) + 2), b"4-byte")
    bad(11, P((1 << 20) + 4), b"8-byte")
    bad(4, 1 << 20, b"2^30")
    out = G.native.fjsp_out()
    assert L.fjsp_step_held(None, a, None, 1, ctypes.byref(out), a) < 0 and b"null handle" in L.fjsp_last_error()
    assert L.fjsp_actions(None, 2, 0, 0, 0, a) < 0 and b"null handle" in L.fjsp_last_error()
    # the arguments are checked before the handle is touched (`a` is no handle)
    assert L.fjsp_step_held(a, a, None, 1, ctypes.byref(out), None) < 0 and b"null held" in L.fjsp_last_error()
    assert L.fjsp_step_held(a, a, None, 1, ctypes.byref(out), P((1 << 20) + 2)) < 0 and b"4-byte" in L.fjsp_last_error()
    assert L.fjsp_actions(a, 2, 0, 0, 0, None) < 0 and b"null actions" in L.fjsp_last_error()
    assert L.fjsp_actions(a, 3, 0, 0, 0, a) < 0 and b"bad action_mode" in L.fjsp_last_error()
