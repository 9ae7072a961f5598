"""Episode accounting on the host: episodes_reference (the specification of fjsp_episode_scan)
against the reference's own recorded rewards, and the entry's argument validation (no GPU)."""
import ctypes

import numpy as np
import pytest

from tests import episodes_util as U
from tests import gpu_util as G

E = U.episodes


def _column_records(name, key):
    c = U.column(name, key)
    recs, acc, ln = U.reference(c)
    return c, recs, acc, ln


def _check_sums(c, recs):
    """by_agent = the segment's rewards summed in step order per agent, total = Python sum() over
    the eight, both bitwise."""
    start = 0
    for r in recs:
        end = int(r["end_step"])
        assert r["length"] == end - start
        seg = c["rewards"][start:end, :, 0]
        by = np.cumsum(seg, axis=0)[-1]
        assert by.tobytes() == r["by_agent"].tobytes()
        assert np.float64(sum(float(x) for x in by)).tobytes() == r["total"].tobytes()
        start = end


@pytest.mark.parametrize("policy", ["unmasked", "masked"])
@pytest.mark.parametrize("seed", U.SEEDS)
def test_random_traces_four_truncated_episodes(policy, seed):
    c, recs, acc, ln = _column_records("traces", f"{policy}_s{seed}")
    assert len(recs) == 4
    assert recs["length"].tolist() == [201] * 4
    assert recs["end_step"].tolist() == [201, 402, 603, 804]
    assert recs["flags"].tolist() == [E.FLAG_TRUNCATED] * 4
    assert recs["seq"].tolist() == [0, 1, 2, 3] and recs["env_gid"].tolist() == [0] * 4
    _check_sums(c, recs)
    # the open episode's carry: the 196 rows after the last end
    assert ln.tolist() == [196]
    assert acc[:, 0].tobytes() == np.cumsum(c["rewards"][804:, :, 0], axis=0)[-1].tobytes()


def test_heuristic_traces_terminated_episodes():
    counts = []
    for seed in U.SEEDS:
        c, recs, _, _ = _column_records("traces", f"heuristic_s{seed}")
        counts.append(len(recs))
        assert (recs["flags"] == E.FLAG_TERMINATED).all()
        assert recs["length"].min() >= 30 and recs["length"].max() <= 194
        assert (recs["orders_completed"] == 2).all()
        assert (recs["packaged"] == c["packaged"][recs["end_step"] - 1, 0]).all()
        _check_sums(c, recs)
    assert counts == [11, 11, 10, 7]


def test_trace_slab_has_71_episodes_in_row_major_order():
    recs, _, _ = U.trace_reference()
    assert len(recs) == 71
    assert recs["seq"].tolist() == list(range(71))
    key = list(zip(recs["end_step"].tolist(), recs["env_gid"].tolist()))
    assert key == sorted(key)
    # each column's records equal the column scanned alone, except env id and seq
    names = [f"{p}_s{s}" for p in U.POLICIES for s in U.SEEDS]
    for e, name in enumerate(names):
        _, alone, _, _ = _column_records("traces", name)
        mine = recs[recs["env_gid"] == e].copy()
        mine["env_gid"] = 0
        mine["seq"] = alone["seq"]
        assert mine.tobytes() == alone.tobytes()


def test_short_traces():
    c3, r3, _, _ = _column_records("scenarios", "short_heur_s3")
    c11, r11, _, _ = _column_records("scenarios", "short_heur_s11")
    assert len(r3) == 4 and len(r11) == 5
    assert r3["end_step"].tolist() == [31, 62, 93, 124]
    _check_sums(c3, r3)
    _check_sums(c11, r11)


@pytest.mark.parametrize("rows", U.SPLITS)
def test_splitting_with_the_carry_gives_the_same_records(rows):
    slab = U.trace_slab()
    whole, acc_w, len_w = U.trace_reference()
    parts, acc, ln = [], None, None
    for lo, hi in U.cuts(1000, rows):
        r, acc, ln = U.reference(U.rows_of(slab, lo, hi), acc=acc, length=ln, step0=lo,
                                 seq0=sum(len(p) for p in parts))
        parts.append(r)
    got = np.concatenate(parts)
    assert got.tobytes() == whole.tobytes()
    assert acc.tobytes() == acc_w.tobytes() and ln.tolist() == len_w.tolist()


def test_reference_offsets_and_missing_infos():
    slab = U.synthetic_slab(5)
    recs, _, _ = U.reference(slab, infos=False, step0=100, env_gid0=7, seq0=3)
    base, _, _ = U.reference(slab)
    assert (recs["orders_completed"] == -1).all() and (recs["packaged"] == -1).all()
    assert (recs["end_step"] == base["end_step"] + 100).all()
    assert (recs["env_gid"] == base["env_gid"] + 7).all()
    assert (recs["seq"] == base["seq"] + 3).all()
    assert recs["total"].tobytes() == base["total"].tobytes()
    d = E.records_dict(recs, dropped=2)
    assert d["by_agent"].shape == (8, len(recs)) and d["dropped"] == 2
    assert (d["terminated"] | d["truncated"]).all()


def test_episode_entries_validate_arguments_without_gpu():
    """fjsp_episode_scan / fjsp_episode_temp_bytes (ABI 12 additions) reject null buffers, empty
    shapes, a negative capacity, a short temp buffer and unaligned records before any launch."""
    L = G.native.lib()
    P = ctypes.c_void_p
    a = P(1 << 20)
    n = ctypes.c_uint64()
    assert L.fjsp_episode_temp_bytes(256, 4096, ctypes.byref(n)) == 0
    need = n.value
    assert need >= 256 * 64 * 4 + 8
    assert L.fjsp_episode_temp_bytes(1, 1, ctypes.byref(n)) == 0 and n.value > 0
    assert L.fjsp_episode_temp_bytes(0, 4, ctypes.byref(n)) != 0 and b"must be > 0" in L.fjsp_last_error()
    assert L.fjsp_episode_temp_bytes(4, -1, ctypes.byref(n)) != 0
    assert L.fjsp_episode_temp_bytes(4, 4, None) != 0 and b"null" in L.fjsp_last_error()
    assert L.fjsp_episode_temp_bytes(1 << 20, 1 << 20, ctypes.byref(n)) != 0 and b"2^31" in L.fjsp_last_error()
    #       rewards term trunc oc pk T    N     gid step acc len recs cap count temp bytes stream
    ok = [a, a, a, None, None, 256, 4096, 0, 0, a, a, a, 100, a, a, need, None]

    def bad(i, v, msg):
        b = list(ok)
        b[i] = v
        assert L.fjsp_episode_scan(*b) < 0 and msg in L.fjsp_last_error(), (i, v, L.fjsp_last_error())
    for i in (0, 1, 2, 9, 10, 11, 13, 14):
        bad(i, None, b"null")
    bad(5, 0, b"must be > 0")
    bad(5, -3, b"must be > 0")
    bad(6, 0, b"must be > 0")
    bad(12, -1, b"cap must be >= 0")
    bad(15, need - 1, b"temp buffer too small")
    bad(15, 0, b"temp buffer too small")
    bad(11, P((1 << 20) + 8), b"16-byte aligned")
    bad(5, 1 << 20, b"2^31")
