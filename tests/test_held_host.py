"""CPU check of fjsp_env.h's held_words (the held-tray words fjsp_step_held stores), compiled for
the host through tests/hostsim/held_shim.cpp (TEST-ONLY).

The host build of the state machine replays each recorded run of the reference (traces.npz's
actions, schedule.npz's order tables): its result words and flags must be the recording's, and
held_words of the state after each step and before the reset must equal the words the fixture
built from the reference's objects, row for row; the call must leave the state, its status word
included, as it is.  On constructed states the code bits a SIGNAL and a drop leave behind must
read as 0."""
import ctypes

import numpy as np
import pytest

from tests import hostsim_build as HB
from tests import schedule_util as SU

HOLDS, BUSY = 1 << 13, 1 << 14


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = HB.build_shim(tmp_path_factory.mktemp("held"), HB.source("held_shim.cpp"), "held")
    P = ctypes.c_void_p
    lib.held_replay.restype = None
    lib.held_replay.argtypes = [P, P, P, P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, ctypes.POINTER(ctypes.c_int64)]
    lib.held_cases.restype = None
    lib.held_cases.argtypes = [ctypes.c_int, P, P, ctypes.POINTER(ctypes.c_int)]
    return lib


@pytest.mark.parametrize("policy,seed", SU.RUNS)
def test_replay_equals_the_reference_objects(shim, policy, seed):
    r = SU.run(policy, seed)
    T = len(r["actions"])
    arr = lambda x, dt: np.ascontiguousarray(x, dtype=dt)  # noqa: E731
    actions, results = arr(r["actions"], np.uint8), arr(r["results"][:, :, 0], np.uint32)
    term, trunc, orders = arr(r["term"][:, 0], np.uint8), arr(r["trunc"][:, 0], np.uint8), arr(r["orders"], np.uint8)
    held = np.full((T, 3), 0xDEADBEEF, np.uint32)
    out = (ctypes.c_int64 * 5)()
    shim.held_replay(actions.ctypes.data, results.ctypes.data, term.ctypes.data, trunc.ctypes.data, orders.ctypes.data,
                     orders.shape[0], orders.shape[1], T, held.ctypes.data, out)
    assert out[0] == 0 and out[1] == 0, "the host replay left the recording"
    assert out[2] == int((term | trunc).astype(bool).sum()) == orders.shape[0] - 1
    assert out[3] == 0, "held_words changed the state"
    want = r["held"][:, :, 0]
    assert held.tobytes() == want.tobytes(), np.argwhere(held != want)[:5]
    # not a comparison of zeros: the run holds trays on the AGV and on a machine, busy and not
    assert (want[:, 0] & HOLDS).any() and (want[:, 1:] & HOLDS).any() and (want[:, 1:] & BUSY).any()
    assert ((want[:, 1:] & (HOLDS | BUSY)) == HOLDS).any()


@pytest.mark.parametrize("code", [3 | (2 << 6) | (4 << 10), 0 | (0 << 6) | (1 << 10), 63 | (4 << 6) | (5 << 10)])
def test_stale_code_bits_read_as_zero(shim, code):
    v = np.zeros((6, 3), np.uint32)
    raw = np.zeros(6, np.uint32)
    ok = ctypes.c_int()
    shim.held_cases(code, v.ctypes.data, raw.ctypes.data, ctypes.byref(ok))
    assert ok.value == 1
    assert v[0].tolist() == [1 << 16, 0, HOLDS | code]              # AGV at pickup; the big machine holds, idle
    assert raw[1] == code and v[1].tolist() == [1 << 16, 0, 0]      # after SIGNAL: stale code, word 0
    assert v[2].tolist() == [HOLDS | code | (3 << 16), 0, 0]        # carrying at the small machine
    assert raw[3] == code and v[3].tolist() == [3 << 16, 0, 0]      # after the drop: stale code, no code bits
    assert raw[4] == code & 0x3FF
    assert v[4].tolist() == [HOLDS | (3 << 16), HOLDS, 0]           # empty trays: no order, no start
    assert v[5].tolist() == [1 << 16, 0, 0]                         # fresh env
