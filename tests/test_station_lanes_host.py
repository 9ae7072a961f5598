"""CPU check of the packaging wave's lane-group form (csrc/fjsp_env.h: pack_lane_*, the K wave of
k_step_ag), compiled for the host through tests/hostsim/station_lanes_shim.cpp (TEST-ONLY).

With G = 64 / EPW lane groups, group g of an env holds stations p * G + g in the station slots p of
its own Env and the groups run side by side; their orders-completed / products-packaged counts are
summed, the status bits and the drop's room bits ORed.  Here the G lanes of an env run one after
another and must leave every state word, table byte, result word and snapshot word as the S = 0..3
sequence on one Env does (pack_due / pack_complete, agv_pack_drop, pack_execute / pack_finish): (a)
on a constructed product of station states, actions and drops, (b) in a replay of random episodes,
which is also compared with the plain step.  The shim counts on the sequence alone what the inputs
contain, so a pass on nothing fails."""
import ctypes

import pytest

from tests import hostsim_build as HB

GROUPS = [4, 2, 1]   # 16, 32, 64 envs per workgroup


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = HB.build_shim(tmp_path_factory.mktemp("station_lanes"), HB.source("station_lanes_shim.cpp"), "stationlanes")
    I64P = ctypes.POINTER(ctypes.c_int64)
    lib.lanes_sweep.restype = None
    lib.lanes_sweep.argtypes = [ctypes.c_int, I64P, ctypes.c_char_p, ctypes.c_int]
    lib.lanes_replay.restype = None
    lib.lanes_replay.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                 I64P, ctypes.c_char_p, ctypes.c_int]
    return lib


@pytest.mark.parametrize("groups", GROUPS)
def test_constructed_sweep(shim, groups):
    """Each station empty / queued / a two-run batch due / due with a run queued behind / in flight
    / in flight and full, x actions 0-2 per station x no drop or a drop of each colour (pkg_cap 6).
    The batches split every order over two stations, so with two neighbours due an order completes
    by runs of two stations in one step; a full station sends a BLUE drop to the second BLUE
    station, and a drop whose stations are all full is lost."""
    out = (ctypes.c_int64 * 9)()
    msg = ctypes.create_string_buffer(512)
    shim.lanes_sweep(groups, out, msg, len(msg))
    cases, bad, two_stations, order_by_two, d0, d1, d2, d3, lost = out
    assert cases == 6 ** 4 * 81 * 4
    assert bad == 0, msg.value.decode()
    assert two_stations > 0 and order_by_two > 0
    assert d0 > 0 and d1 > 0 and d2 > 0 and d3 > 0 and lost > 0


# num_orders -> what the S = 0..3 sequence meets with seed 11, 32 envs x 450 steps of uniform-random
# actions: (steps with completions at two stations, orders completed by two stations' runs in one
# step, drops to station 0..3, drops lost).  Random play drops a tray at packaging about once in 600
# env-steps, to the first station of its colour, and never has two stations busy at once: the events
# it does not reach are the constructed sweep's.
REPLAY = {2: (0, 0, 7, 0, 5, 14, 0), 30: (0, 0, 9, 0, 6, 8, 0)}


@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("num_orders", sorted(REPLAY))
def test_replay(shim, groups, num_orders):
    """32 envs x 450 steps of uniform-random actions with auto-reset at 2 and at 30 orders: K's words
    live on the lane groups from reset to reset (the wave's own reset of its lanes included), every
    env-step compared with the sequence and with the plain step."""
    out = (ctypes.c_int64 * 10)()
    msg = ctypes.create_string_buffer(512)
    shim.lanes_replay(groups, 32, 450, num_orders, 20, 11, out, msg, len(msg))
    compared, bad, resets = out[0], out[1], out[2]
    events = tuple(out[3:10])
    assert compared == 32 * 450
    assert bad == 0, msg.value.decode()
    assert resets >= 32 * 2            # the 201-step truncation at least
    assert sum(events[2:6]) > 0 and sum(1 for d in events[2:6] if d > 0) >= 2
    assert events == REPLAY[num_orders], events
