"""CPU check of fjsp_orders.h's put_orders_env (the per-env work of fjsp_put_orders), compiled for
the host with the state machine through tests/hostsim/orders_shim.cpp (TEST-ONLY).

The host build replays every run of tests/golden/orders.npz (recorded from the reference on
caller-chosen order books and with generate_order calls between steps, one after the episode had
terminated): the book goes in through put_orders_env(append = 0), each arrival through
put_orders_env(append = 1), the recorded actions through env_step, and every recorded word must
come out equal.  Single calls on a caller-held world check that each invalid kind leaves the env
byte-equal and that a valid append changes only W0's count field and the new order rows.  The same
shim is built once more with a stand-alone main under -fsanitize=address,undefined and run."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import hostsim_build as HB

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "orders.npz")
RUNS = ["one", "nine", "full", "one_heur", "arrivals"]
P = ctypes.c_void_p


class OrdersRun(ctypes.Structure):   # struct OrdersRun of orders_shim.cpp
    _fields_ = [("book", P), ("arrivals", P), ("actions", P), ("K", ctypes.c_int32), ("n_arr", ctypes.c_int32),
                ("T", ctypes.c_int32), ("pad", ctypes.c_int32)] + \
               [(k, P) for k in ("init_i32", "init_i8", "init_f32", "init_mk", "arr_i32", "arr_i8", "arr_f32", "arr_mk",
                                 "arr_id", "i32", "i8", "f32", "mk", "rew", "term", "trunc", "res", "sim_time", "oc",
                                 "pk")] + \
               [("status", ctypes.c_uint32), ("rejected", ctypes.c_int32)]


def word(n, ty, co):
    return n | (ty << 4) | (co << 6)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = HB.build_shim(tmp_path_factory.mktemp("orders"), HB.source("orders_shim.cpp"), "orders")
    lib.orders_replay.restype = None
    lib.orders_replay.argtypes = [ctypes.POINTER(OrdersRun)]
    lib.orders_world_bytes.restype = ctypes.c_int
    lib.orders_world_layout.restype = None
    lib.orders_world_layout.argtypes = [P]
    lib.orders_put.restype = ctypes.c_int
    lib.orders_put.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.orders_world_run.restype = ctypes.c_uint32
    lib.orders_world_run.argtypes = [P, ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.mark.parametrize("run", RUNS)
def test_replay_equals_the_reference(shim, gold, run):
    g = {k[len(run) + 1:]: gold[k] for k in gold.files if k.startswith(run + "_") and
         (run != "one" or not k.startswith("one_heur_"))}
    T = int(g["meta"][3])
    book = np.array([word(*map(int, o)) for o in g["book"]], np.uint32)
    arr = np.ascontiguousarray(g.get("arrivals", np.zeros((0, 7), np.int64)), dtype=np.int64)
    n = len(arr)
    actions = np.ascontiguousarray(g["actions"], dtype=np.uint8)
    shapes = {"init_i32": ((20,), np.int32), "init_i8": ((12,), np.int8), "init_f32": ((6,), np.float32),
              "init_mk": ((29,), np.int8), "arr_i32": ((n, 20), np.int32), "arr_i8": ((n, 12), np.int8),
              "arr_f32": ((n, 6), np.float32), "arr_mk": ((n, 29), np.int8), "arr_id": ((n,), np.int32),
              "i32": ((T, 20), np.int32), "i8": ((T, 12), np.int8), "f32": ((T, 6), np.float32),
              "mk": ((T, 29), np.int8), "rew": ((T, 8), np.float64), "term": ((T,), np.uint8),
              "trunc": ((T,), np.uint8), "res": ((T, 8), np.uint32), "sim_time": ((T,), np.float64),
              "oc": ((T,), np.int32), "pk": ((T,), np.int32)}
    out = {k: np.frombuffer(bytearray(b"\x5a" * (max(int(np.prod(s)), 1) * np.dtype(dt).itemsize)), dtype=dt)
           for k, (s, dt) in shapes.items()}   # prefilled: a field the replay skipped cannot pass
    r = OrdersRun(book=book.ctypes.data, arrivals=arr.ctypes.data, actions=actions.ctypes.data, K=len(book), n_arr=n, T=T)
    for k in shapes:
        setattr(r, k, out[k].ctypes.data)
    shim.orders_replay(ctypes.byref(r))
    assert r.rejected == 0 and r.status == 0
    want = {"init_i32": "init_i32", "init_i8": "init_i8", "init_f32": "init_f32", "init_mk": "init_masks",
            "i32": "obs_i32", "i8": "obs_i8", "f32": "obs_f32", "mk": "masks", "rew": "rewards", "term": "term",
            "trunc": "trunc", "res": "results", "sim_time": "sim_time", "oc": "orders_completed", "pk": "packaged"}
    if n:
        want.update({"arr_i32": "arr_i32", "arr_i8": "arr_i8", "arr_f32": "arr_f32", "arr_mk": "arr_masks"})
        assert out["arr_id"][:n].tolist() == arr[:, 5].tolist()
    for mine, theirs in want.items():
        s, dt = shapes[mine]
        got = out[mine][:int(np.prod(s))].reshape(s)
        ref = np.ascontiguousarray(g[theirs]).astype(dt)
        assert (ref == g[theirs]).all() and got.shape == ref.shape, (mine, got.shape, ref.shape)
        assert got.tobytes() == ref.tobytes(), (run, mine, np.argwhere(got != ref)[:5])


def test_the_fixture_holds_what_it_was_specified_with(gold):
    assert gold["one_book"].tolist() == [[1, 2, 3]] and gold["nine_book"][0, 0] == 9 and len(gold["full_book"]) == 64
    assert all(int(gold[f"{r}_meta"][3]) == 120 for r in ("one", "nine", "full"))
    assert gold["one_heur_term"][-1] == 1 and gold["one_heur_term"][:-1].sum() == 0
    arr, term = gold["arrivals_arrivals"], gold["arrivals_term"]
    assert arr[:, 1].tolist() == [0, 3, 0] and arr[1, 2] == 3 and arr[:, 5].tolist() == [1, 2, 3]
    t = int(arr[2, 0])                       # the arrival after the episode had terminated: 1 -> 0 -> ... -> 1
    assert term[t - 1] == 1 and term[t] == 0 and term[-1] == 1 and gold["arrivals_orders_completed"][-1] == 4
    # the first came with the queue empty and the station idle, the second with an order half loaded
    i32 = gold["arrivals_obs_i32"]
    assert i32[int(arr[0, 0]) - 1, 0] == 0 and 0 < i32[int(arr[1, 0]) - 1, 1] < i32[int(arr[1, 0]) - 1, 0]


# ---------------------------------------------------------------- single calls
class World:
    def __init__(self, shim, book=((3, 1, 2), (9, 2, 1), (2, 3, 3)), steps=12):
        self.shim = shim
        self.buf = np.zeros(shim.orders_world_bytes(), np.uint8)
        lay = np.zeros(5, np.int32)
        shim.orders_world_layout(lay.ctypes.data)
        self.w_off, self.nw, self.pg_off, self.o_off, self.no = map(int, lay)
        src = np.array([word(*o) for o in book], np.uint32)
        assert self.put(src, len(src), len(src), 0) == 1
        assert shim.orders_world_run(self.buf.ctypes.data, steps) == 0
        self.buf[self.pg_off:self.pg_off + 4].view(np.uint32)[0] = 0x0500_0001   # a pre-drawn table on record

    def put(self, src, K, count, append, stride=1):
        src = np.ascontiguousarray(src, dtype=np.uint32)
        return self.shim.orders_put(self.buf.ctypes.data, src.ctypes.data, stride, K, count, append)

    @property
    def words(self):
        return self.buf[self.w_off:self.w_off + 4 * self.nw].view(np.uint32)

    @property
    def orders(self):
        return self.buf[self.o_off:self.o_off + 4 * self.no].view(np.uint32)


GOOD = word(4, 2, 2)
INVALID = {
    "n = 0": ([GOOD, word(0, 1, 1)], 2, 2),
    "n = 10": ([word(10, 1, 1)], 1, 1),
    "type 0": ([GOOD, GOOD, word(3, 0, 2)], 3, 3),
    "type 4 via high bits": ([4 | (4 << 4) | (1 << 8)], 1, 1),
    "colour 0": ([word(3, 2, 0)], 1, 1),
    "a stray high bit": ([GOOD | (1 << 31)], 1, 1),
    "count < 0": ([GOOD], 1, -1),
    "count > K": ([GOOD, GOOD], 2, 3),
}


@pytest.mark.parametrize("append", [0, 1])
@pytest.mark.parametrize("kind", list(INVALID))
def test_an_invalid_env_is_left_byte_equal(shim, kind, append):
    W = World(shim)
    before = W.buf.copy()
    src, K, count = INVALID[kind]
    assert W.put(src + [GOOD], K, count, append) == 0
    assert W.buf.tobytes() == before.tobytes()


def test_an_append_past_64_is_rejected_and_64_is_not(shim):
    W = World(shim)
    src = np.full(64, GOOD, np.uint32)
    before = W.buf.copy()
    assert W.put(src, 64, 62, 1) == 0 and W.buf.tobytes() == before.tobytes()
    assert W.put(src, 64, 61, 1) == 1 and (W.words[0] >> 16) & 0xFF == 64
    before = W.buf.copy()
    assert W.put(src, 1, 1, 1) == 0 and W.buf.tobytes() == before.tobytes()
    assert W.put(src, 64, 0, 1) == 1                      # nothing arrives: valid
    assert W.put(src, 64, 64, 0) == 1 and (W.words[0] >> 16) & 0xFF == 64


def test_a_valid_append_changes_only_the_count_and_the_new_rows(shim):
    W = World(shim)
    before = W.buf.copy()
    w0, orders0 = W.words.copy(), W.orders.copy()
    src = np.zeros((2, 7), np.uint32)                    # column 3 of a [2][7] table
    src[:, 3] = [word(9, 3, 1), word(1, 1, 3)]
    assert W.put(src.reshape(-1)[3:], 2, 2, 1, stride=7) == 1
    assert W.words[0] == (w0[0] & ~np.uint32(0xFF << 16)) | np.uint32(5 << 16)
    assert (W.words[1:] == w0[1:]).all()
    assert (W.orders[:3] == orders0[:3]).all() and (W.orders[5:] == orders0[5:]).all()
    assert W.orders[3:5].tolist() == [(9 << 20) | (3 << 24) | (1 << 26), (1 << 20) | (1 << 24) | (3 << 26)]
    # outside the count field, the new rows and the dropped pre-draw record the world is byte-equal
    after = W.buf.copy()
    for off, n in ((W.w_off, 4), (W.o_off + 12, 8), (W.pg_off, 4)):
        after[off:off + n] = before[off:off + n]
    assert after.tobytes() == before.tobytes()
    assert W.buf[W.pg_off:W.pg_off + 4].view(np.uint32)[0] == 0


def test_a_reset_keeps_the_cursor_and_clears_the_rest(shim):
    W = World(shim)
    W.words[3] = 0x8123_0042
    fresh = World(shim, book=((2, 2, 2),), steps=0)
    fresh.words[3] = 0x8123_0042
    assert W.put([word(2, 2, 2)], 1, 1, 0) == 1
    assert W.words.tobytes() == fresh.words.tobytes() and W.orders[0] == fresh.orders[0]
    assert W.buf[W.pg_off:W.pg_off + 4].view(np.uint32)[0] == 0
    assert W.put([], 0, 0, 0) == 1 and (W.words[0] >> 16) == 0          # the empty episode


def test_sanitized_standalone_run(tmp_path):
    exe = HB.build_program(tmp_path, [HB.source("orders_san_main.cpp")], sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().endswith("OK")
