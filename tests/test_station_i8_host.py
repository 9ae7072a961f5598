"""CPU check of fjsp_env.h's station_i8 (the stations' is_busy / queue_length of a state without
observing it: k_policy_step's KPI output obs_i8), compiled for the host through
tests/hostsim/station_i8_shim.cpp (TEST-ONLY).

Its twelve values must be what observe() hands its sink's i8(), truncated to int8 as the sinks
store them, on every state a rollout with auto-reset visits and on a constructed state whose queue
words are above 127; and it must leave the state, its status word included, as it is."""
import ctypes

import numpy as np
import pytest

from tests import hostsim_build as HB


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = HB.build_shim(tmp_path_factory.mktemp("station_i8"), HB.source("station_i8_shim.cpp"), "stationi8")
    lib.station_i8_replay.restype = None
    lib.station_i8_replay.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                      ctypes.POINTER(ctypes.c_int64)]
    lib.station_i8_case.restype = None
    lib.station_i8_case.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    return lib


@pytest.mark.parametrize("num_orders", [2, 30])
def test_replay_equals_observe(shim, num_orders):
    """32 envs x 450 steps of uniform-random actions with auto-reset: after every step (the state
    before the reset, which the step kernels emit obs_i8 from) and after every reset the helper's
    twelve values equal observe()'s.  The rollout must reach busy machines and waiting trays, so
    that the comparison is not one of zeros."""
    out = (ctypes.c_int64 * 15)()
    shim.station_i8_replay(32, 450, num_orders, 11, out)
    compared, bad, resets = out[0], out[1], out[2]
    nonzero = list(out[3:15])
    assert resets >= 32 * 2                      # the 201-step truncation at least
    assert compared == 32 * 450 + resets
    assert bad == 0
    # both machines' is_busy (fields 0, 2) and queue_length (1, 3) were non-zero somewhere
    assert all(nonzero[f] > 0 for f in (0, 1, 2, 3)), nonzero


@pytest.mark.parametrize("q0,q1,qp,busy", [(200, 128, 127, 1), (127, 255, 300, 0), (3, 0, 129, 1), (256, 383, 16000, 1)])
def test_queue_words_above_127_wrap_as_int8(shim, q0, q1, qp, busy):
    """A constructed state with queue words above 127: the helper wraps them as (int8_t), as
    obs_i8_checked does, and sets no status bit (observe() flags the overflow, the helper must
    not: the status the collect emits is the step's)."""
    got, want = np.zeros(12, np.int8), np.zeros(12, np.int8)
    status = (ctypes.c_uint32 * 2)()
    shim.station_i8_case(q0, q1, qp, busy, got.ctypes.data, want.ctypes.data, status)
    wrap = lambda v: ((v + 128) & 0xFF) - 128  # noqa: E731
    expect = [busy, wrap(q0), busy, wrap(q1)] + [x for s in range(4) for x in (busy, wrap(qp + s))]
    assert got.tolist() == expect
    assert want.tolist() == expect
    assert status[0] == 0
    assert (status[1] != 0) == (max(q0, q1, qp + 3) > 127)
